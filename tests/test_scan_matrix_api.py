"""CPU-side checks of option "scan_matrix" (hnsw_scan_matrix.hip): scan-path value 3 is named in the header and the three front
ends with the ABI version unchanged, the sources are in the build, and the plan header's arithmetic and screening rule hold."""
import importlib.util
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_option_and_scan_path_3_are_declared_and_mirrored():
    import ocaml_hnsw_amd as H
    hdr = open(os.path.join(ROOT, "include", "hnsw_mi355x.h")).read()
    assert '"scan_matrix"' in hdr and "3 the float matrix scan" in hdr
    assert re.search(r"#define\s+HNSW_ABI_VERSION\s+3\b", hdr) and H.ABI_VERSION == 3       # an additive option
    assert H.SCAN_PATH_MATRIX == 3 and "scan_matrix" in H.Hgraph.set_option.__doc__
    for path, text in (("csrc/hnsw_scan_matrix_plan.h", "SCAN_PATH_MATRIX = 3;"), ("ocaml/hnsw_mi355x.ml", "let scan_path_matrix = 3"), ("host/hnsw_front.hpp", "SCAN_PATH_MATRIX = 3;")):
        assert text in open(os.path.join(ROOT, "ocaml-hnsw_amd", path)).read(), path
    spec = importlib.util.spec_from_file_location("hnsw_build", os.path.join(ROOT, "ocaml-hnsw_amd", "build.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    assert "hnsw_scan_matrix.hip" in b.SOURCES and "hnsw_scan_matrix.hip" in b.DEPS and "hnsw_scan_matrix_plan.h" in b.DEPS


def test_scan_matrix_plan(tmp_path):
    """tests/cpp/test_scan_matrix_plan.cpp, a host program, under AddressSanitizer and UndefinedBehaviorSanitizer"""
    exe = str(tmp_path / "test_scan_matrix_plan")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "cpp", "test_scan_matrix_plan.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and re.search(r"scan matrix plan ok: [1-9]\d* cases, 0 failed", out.stdout), out.stdout + out.stderr
