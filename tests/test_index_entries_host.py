"""CPU suite: csrc/index_entries.h on its own: the size of an index, the entries that wait for their
window, the job list of an indexed batch decode, the rule that cuts every encoder's bands at the entry rows and the rule that
says which image of a batch gets an index.  tools/index_entries_check.cpp checks them -- the band rule exhaustively over
1 <= h <= 40, 1 <= band <= h, 0 <= every <= h + 1 -- and is built and run here."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_standalone_check_under_sanitizers(tmp_path):
    """tools/index_entries_check.cpp: index_entries.h alone, with its own main, under the address and undefined-behaviour
    sanitizers (nothing of it is loaded into Python)."""
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "index_entries_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                    os.path.join(ROOT, "tools", "index_entries_check.cpp")], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "index_entries_check ok" in r.stdout
