"""CPU-side checks of the range scan's matrix form (hnsw_range_matrix.hip, option "scan_matrix"): the source is in the build, the
documentation of the scan path names range calls, and the plan header's arithmetic and the range rule hold."""
import importlib.util
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_source_is_built_and_the_scan_path_speaks_of_range_calls():
    import ocaml_hnsw_amd as H
    spec = importlib.util.spec_from_file_location("hnsw_build", os.path.join(ROOT, "ocaml-hnsw_amd", "build.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    assert "hnsw_range_matrix.hip" in b.SOURCES and "hnsw_range_matrix.hip" in b.DEPS and "hnsw_scan_matrix_device.hip.h" in b.DEPS
    assert "range" in H.Hgraph.scan_path.__doc__


def test_range_matrix_plan(tmp_path):
    """tests/cpp/test_range_matrix_plan.cpp, a host program, under AddressSanitizer and UndefinedBehaviorSanitizer"""
    exe = str(tmp_path / "test_range_matrix_plan")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "cpp", "test_range_matrix_plan.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and re.search(r"range matrix plan ok: [1-9]\d* cases, 0 failed", out.stdout), out.stdout + out.stderr
