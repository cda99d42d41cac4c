"""CPU-side checks of option "scan_bytes" (ocaml-hnsw_amd/csrc/hnsw_scan_bytes.hip): hnsw_index_scan_path is declared, exported and
mirrored in the three front ends with the ABI version unchanged, and the plan header's arithmetic holds."""
import ctypes
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_scan_path_is_declared_exported_and_mirrored():
    import ocaml_hnsw_amd as H
    hdr = open(os.path.join(ROOT, "include", "hnsw_mi355x.h")).read()
    assert re.search(r"int32_t hnsw_index_scan_path\(hnsw_index \*idx, int32_t \*out\);", hdr) and '"scan_bytes"' in hdr
    assert re.search(r"#define\s+HNSW_ABI_VERSION\s+3\b", hdr) and H.ABI_VERSION == 3       # an additive entry point
    assert "hnsw_index_scan_path" in H.ABI_SYMBOLS and callable(H.Hgraph.scan_path)
    fn = H.load().hnsw_index_scan_path
    assert len(fn.argtypes) == 2 and fn.restype is ctypes.c_int32
    out = ctypes.c_int32(7)
    assert fn(None, ctypes.byref(out)) == H.ERR_BAD_ARG and out.value == 7        # refused on the host, nothing written
    ml = open(os.path.join(ROOT, "ocaml-hnsw_amd", "ocaml", "hnsw_mi355x.ml")).read()
    hpp = open(os.path.join(ROOT, "ocaml-hnsw_amd", "host", "hnsw_front.hpp")).read()
    assert re.search(r'foreign[^"]*"hnsw_index_scan_path"', ml) and "let scan_path " in ml
    assert "hnsw_index_scan_path(" in hpp and " scan_path(" in hpp
    import importlib.util
    spec = importlib.util.spec_from_file_location("hnsw_build", os.path.join(ROOT, "ocaml-hnsw_amd", "build.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    assert "hnsw_scan_bytes.hip" in b.SOURCES and "hnsw_scan_bytes.hip" in b.DEPS and "hnsw_scan_bytes_plan.h" in b.DEPS


def test_scan_bytes_plan(tmp_path):
    """tests/cpp/test_scan_bytes_plan.cpp, a host program, under AddressSanitizer and UndefinedBehaviorSanitizer"""
    exe = str(tmp_path / "test_scan_bytes_plan")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "cpp", "test_scan_bytes_plan.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    done = re.search(r"scan bytes plan ok: (\d+) cases, 0 failed", out.stdout)
    assert out.returncode == 0 and done and int(done.group(1)) > 0, out.stdout + out.stderr
