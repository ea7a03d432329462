"""CPU suite: the copy engine's host logic (csrc/copy_engine.h).  The chunk ring of code_packs, the
fallback to the runtime's copies and the loader are driven by tools/copy_engine_check.cpp with a fake engine; nothing of
it is loaded into Python and no call touches a GPU."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_symbol_exported_and_declared(pkg):
    lib = pkg.load_library()
    text = open(pkg.INCLUDE).read()
    assert hasattr(lib, "nblic_amd_copy_stats") and "nblic_amd_copy_stats" in pkg.EXPORTS
    assert re.search(r"\bnblic_amd_copy_stats\s*\(", text)
    assert lib.nblic_amd_copy_stats(None, None) == -1


def test_no_hip_in_the_interface():
    """copy_engine.h is host-only: it compiles without the HIP headers (the stand-alone check does just that) and names
    no HIP type."""
    text = open(os.path.join(ROOT, "nblic-image-compression_amd", "csrc", "copy_engine.h")).read()
    assert "#include <hip" not in text and not re.search(r"\bhip[A-Z]\w*_t\b", text)


def test_standalone_check_under_sanitizers(tmp_path):
    """tools/copy_engine_check.cpp: copy_engine.h alone, with its own main, under the address and undefined-behaviour
    sanitizers: 1-3 packs, 1-9 chunks, lanes of unequal length, an error injected at every call in turn, the library
    that is not there."""
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "copy_engine_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-pthread", "-o", exe,
                    os.path.join(ROOT, "tools", "copy_engine_check.cpp"), "-ldl"], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr[-4000:]
    assert "copy_engine_check ok" in r.stdout
