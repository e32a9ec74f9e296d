"""The packed-input layouts of the local map's calls (mcorb_pack.h) as a stand-alone program under the sanitizers.  No GPU.

On the commit before the header existed the program does not compile."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_layouts_under_asan_ubsan(tmp_path):
    """tests/cpp/test_pack_sanitize.cpp (its own main, plain g++, -fsanitize=address,undefined): the five blocks the library
    builds, with its item types -- every offset a multiple of 32, no overlap, the total covering the last item, an item of no
    elements taking no space; every item is written end to end into a vector of `total` bytes.  No report, bad=0"""
    exe = str(tmp_path / "test_pack_sanitize")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I" + os.path.join(ROOT, "mc-slam_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "test_pack_sanitize.cpp"),
                           "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "bad=0" in out.stdout and not out.stderr, out.stdout + out.stderr
