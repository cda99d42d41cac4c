"""CPU-side checks of option "scan_bytes" 2 (ocaml-hnsw_amd/csrc/hnsw_range_bytes.hip): the source is built, the header says what the
value does, and the plan header's arithmetic (which value serves which scans; the integer bound of a key interval) holds."""
import importlib.util
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_range_bytes_is_built_and_documented():
    spec = importlib.util.spec_from_file_location("hnsw_build", os.path.join(ROOT, "ocaml-hnsw_amd", "build.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    assert "hnsw_range_bytes.hip" in b.SOURCES and "hnsw_range_bytes.hip" in b.DEPS and "hnsw_scan_bytes_plan.h" in b.DEPS
    hdr = open(os.path.join(ROOT, "include", "hnsw_mi355x.h")).read()
    option = hdr[hdr.index('"scan_bytes"    0 (default)'):hdr.index('"scan_matrix"   0 (default)')]
    assert re.search(r"\b2 = ", option) and "range" in option and "profiles/range_bytes.txt" in option


def test_range_bytes_plan(tmp_path):
    """tests/cpp/test_range_bytes_plan.cpp, a host program, under AddressSanitizer and UndefinedBehaviorSanitizer"""
    exe = str(tmp_path / "test_range_bytes_plan")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "cpp", "test_range_bytes_plan.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and re.search(r"range bytes plan ok: [1-9]\d* cases, 0 failed", out.stdout), out.stdout + out.stderr
