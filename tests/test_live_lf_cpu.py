"""mcorb_rig_set_lf (obtainLfFeatures and the LF set's transform inside the extraction job) without a device: the library exports
the calls with the header's signatures and refuses a NULL rig before any device call, the Python and C++ mirrors exist, and the
shared triangulation header (mcorb_triangulate.h, the code k_lf_tracks runs) built by plain g++ equals the library's host
triangulation bit for bit."""
import ctypes as C
import os
import re
import subprocess
from importlib import import_module

import numpy as np
import pytest

import lf_problems

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mc-slam_amd", "csrc")
pkg = import_module("mc-slam_amd")

DECLS = {
    "mcorb_rig_set_lf": r"int mcorb_rig_set_lf\(mcorb_rig \*r, const mcorb_camera \*cams, int total_feats\);",
    "mcorb_rig_get_lf_features": r"int mcorb_rig_get_lf_features\(mcorb_rig \*r, int slot, int frame, mcorb_lf_feature \*out, int cap, "
                                 r"int \*n_out,\s+int \*intramatch_size_out, int \*mono_size_out, uint32_t \*words_fil, int cap_words, "
                                 r"int \*nwords_fil_out\);",
    "mcorb_rig_get_lf_bow": r"int mcorb_rig_get_lf_bow\(mcorb_rig \*r, int slot, int frame, uint32_t \*bow_ids, double \*bow_vals, "
                            r"int bow_cap, int \*nbow,\s+uint32_t \*fv_nodes, int32_t \*fv_offsets, int fv_cap, int \*nfv, "
                            r"int32_t \*fv_feats, int feat_cap\);",
    "mcorb_dev_triangulate_selftest": r"int mcorb_dev_triangulate_selftest\(int device, const double \*x, const double \*P, "
                                      r"const int32_t \*nv, int n, double \*X, int32_t \*branch\);",
}


def test_header_declares_and_library_exports_the_calls():
    src = open(os.path.join(ROOT, "include", "mcorb.h")).read()
    L = pkg._lib.load()
    for name, decl in DECLS.items():
        assert re.search(decl, src), name
        assert hasattr(L, name), name
        nargs = len(re.search(r"\((.*?)\);", re.search(decl, src).group(0), re.S).group(1).split(","))
        assert len(pkg._lib.SIGNATURES[name][1]) == nargs, name


def test_calls_refuse_a_null_rig():
    L, E_ARG = pkg._lib.load(), pkg._lib.E_ARG
    cams = (pkg._lib.Camera * 2)()
    n = C.c_int(7)
    assert L.mcorb_rig_set_lf(None, cams, 3000) == E_ARG
    assert L.mcorb_rig_set_lf(None, None, 0) == E_ARG
    assert L.mcorb_rig_get_lf_features(None, 0, 0, None, 0, C.byref(n), None, None, None, 0, None) == E_ARG
    assert n.value == 0
    assert L.mcorb_rig_get_lf_bow(None, 0, 0, None, None, 0, None, None, None, 0, None, None, 0) == E_ARG
    x, P, nv = np.zeros(4), np.zeros(24), np.array([2], np.int32)
    X, br = np.zeros(3), np.zeros(1, np.int32)
    assert L.mcorb_dev_triangulate_selftest(0, None, P.ctypes.data, nv.ctypes.data, 1, X.ctypes.data, br.ctypes.data) == E_ARG
    nv1 = np.array([1], np.int32)   # a view count out of range is refused before the device is looked for
    assert L.mcorb_dev_triangulate_selftest(0, x.ctypes.data, P.ctypes.data, nv1.ctypes.data, 1, X.ctypes.data, br.ctypes.data) == E_ARG


def test_python_and_adapter_mirrors_exist():
    for m in ("set_lf", "lf_features", "lf_bow"):
        assert callable(getattr(pkg.Rig, m)), m
    assert callable(getattr(pkg.MultiCameraFrame, "setLfConfig"))
    assert callable(getattr(pkg.IntraMatch, "from_lf"))
    hpp = open(os.path.join(ROOT, "include", "mcorb_adapter.hpp")).read()
    assert "void setLfConfig(const std::vector<std::array<double, 9>> &K_mats" in hpp
    assert "void setLfConfig(const std::vector<cv::Mat> &K_mats" in hpp
    for member in ("intraMatches", "intramatch_size", "mono_size", "lfBoW", "lfFeatVec", "matchDesc", "point3D", "uv_ref"):
        assert member in hpp, member


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("tri") / "test_triangulate")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-I" + CSRC,
                           os.path.join(ROOT, "tests", "cpp", "test_triangulate.cpp"), "-o", out])
    return out


def test_header_alone_equals_the_library_bit_for_bit(exe, tmp_path):
    """4000 problems of 2 .. 8 views, every kind: the g++ build of the header and mcorb_host_triangulate(_branch) give the same
    bits, and every exit of the solver is taken"""
    nv, x, P, kinds = lf_problems.problems(4000, 8, seed=11)
    n = len(nv)
    inp, outp = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(inp, "wb") as f:
        f.write(np.int32(n).tobytes())
        f.write(nv.tobytes())
        xo = po = 0
        for k in nv:
            f.write(x[xo:xo + 2 * k].tobytes())
            f.write(P[po:po + 12 * k].tobytes())
            xo += 2 * k
            po += 12 * k
    subprocess.check_call([exe, inp, outp])
    rec = np.fromfile(outp, np.dtype([("X", "<f8", (3,)), ("br", "<i4")]))
    assert len(rec) == n
    L = pkg._lib.load()
    X, X2, br = np.zeros(3), np.zeros(3), np.zeros(1, np.int32)
    xo = po = 0
    for i, k in enumerate(nv):
        xi, Pi = np.ascontiguousarray(x[xo:xo + 2 * k]), np.ascontiguousarray(P[po:po + 12 * k])
        assert L.mcorb_host_triangulate_branch(xi.ctypes.data, Pi.ctypes.data, int(k), X.ctypes.data, br.ctypes.data) == 0
        assert L.mcorb_host_triangulate(xi.ctypes.data, Pi.ctypes.data, int(k), X2.ctypes.data) == 0
        assert X.tobytes() == rec["X"][i].tobytes() == X2.tobytes(), "problem %d (%s, %d views)" % (i, kinds[i], k)
        assert br[0] == rec["br"][i]
        xo += 2 * k
        po += 12 * k
    assert set(rec["br"].tolist()) == {0, 1, 2, 3}, np.bincount(rec["br"])
