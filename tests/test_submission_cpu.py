"""Submission (mc-slam_amd/csrc/mcorb_hip.h), the one mechanism behind "nothing returns between a call's first queued piece and its
wait", as a stand-alone program under the sanitizers against a scripted HIP runtime.  No GPU, no HIP library: the runtime's
declarations are tests/cpp/hipmock's.  The failure path cannot be reached on a device without making a HIP call fail, so this is
where it is held; what the chains compute is held bit for bit by the stores', the estimators' and the tracking tests."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_submission_under_asan_ubsan(tmp_path):
    """tests/cpp/test_submission.cpp (its own main, -fsanitize=address,undefined), on every rotation of the chain mark, run, copy, fill,
    run: with every piece succeeding the log is the pieces in order and one synchronisation, and wait() is MCORB_OK; with piece k
    failing -- a launch by the thread's last error, a copy or fill by its return value, a mark by the event record -- for every k,
    failed() is false up to piece k and true behind it, no later piece reaches the runtime and no later launch lambda is called,
    the synchronisation still happens exactly once and last, and wait() is MCORB_E_HIP with a message that names the piece's kind
    and carries hipGetErrorString; a failed synchronisation is reported in front of a recorded piece; run(spans, i, launch) does not
    launch behind its failed mark; copies and fills of 0 bytes queue nothing; a Submission without a piece does not synchronise"""
    exe = str(tmp_path / "test_submission")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I" + os.path.join(ROOT, "tests", "cpp", "hipmock"), "-I" + os.path.join(ROOT, "mc-slam_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "test_submission.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and out.stdout.strip() == "bad=0" and not out.stderr, out.stdout + out.stderr
