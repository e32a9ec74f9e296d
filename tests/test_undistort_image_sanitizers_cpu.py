"""CPU-only sanitizer run (ASan + UBSan) of mcorb_undistort_image.h through tests/cpp/test_undistort_image.cpp: the header's own
invariants -- maps that point far outside the source and at every border included: no tap is read out of bounds -- and one
strongly distorted camera whose corners leave the source, equal to the numpy restatement."""
import os
import subprocess

import numpy as np

import test_undistort_image_cpu as T
import undistort_image_ref as R


def test_undistort_image_header_under_asan_ubsan(tmp_path):
    exe = T.build_exe(str(tmp_path / "test_undistort_image_san"),
                      ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "bad=0" in out.stdout, out.stdout + out.stderr
    w, h = 160, 120
    K, src = T.camera(w, h), T.image(5, w, h)
    for dist in (T.MODELS[1][1], T.MODELS[5][1], [1e3, 0, 0, 0], [1e300, 0, 0, 0]):
        st, m1, m2, dst = T.run_exe(exe, str(tmp_path), K, dist, src)
        with np.errstate(all="ignore"):
            r1, r2 = R.undistort_map(K, dist, w, h)
        assert st == 0 and np.array_equal(m1, r1) and np.array_equal(m2, r2) and np.array_equal(dst, R.remap(src, r1, r2)[0])
    assert os.path.exists(exe)
