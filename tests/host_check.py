"""tools/webp_host_check.cpp built under ASan + UBSan, once for the whole run: the fixture that tests/test_webp.py and tests/test_png.py share.  The
program is stand-alone (its own main); nothing of it is loaded into Python."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_built = []


@pytest.fixture(scope="module")
def host_check(tmp_path_factory):
    if _built:
        return _built[0]
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("clang++") or shutil.which("c++")
    assert cxx, "no host C++ compiler (g++ / clang++) to build tools/webp_host_check.cpp with"
    exe = tmp_path_factory.mktemp("webp_host") / "webp_host_check"
    cmd = [cxx, "-std=c++20", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "mmgt_amd", "csrc"),
           os.path.join(ROOT, "tools", "webp_host_check.cpp"), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    _built.append(str(exe))
    return _built[0]
