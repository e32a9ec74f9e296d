"""mcorb_rig_set_vocabulary (the BoW stages inside the extraction job): exported by the library, declared by the header with its two
flags and its LDS bound, bound in Python, and refused without a rig -- all without a device."""
import ctypes as C
import os
import re
from importlib import import_module

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pkg = import_module("mc-slam_amd")


def test_library_exports_set_vocabulary():
    L = pkg._lib.load()
    assert hasattr(L, "mcorb_rig_set_vocabulary")
    assert pkg._lib.SIGNATURES["mcorb_rig_set_vocabulary"][1][3] is C.c_double
    assert L.mcorb_rig_set_vocabulary(None, None, 4, 0.85, 0) == pkg._lib.E_ARG   # no rig: refused before any device call


def test_header_declares_the_call_and_its_flags():
    src = open(os.path.join(ROOT, "include", "mcorb.h")).read()
    assert re.search(r"int mcorb_rig_set_vocabulary\(mcorb_rig \*r, mcorb_vocab \*v, int levelsup, double max_neighbor_ratio, int flags\);", src)
    defs = dict(re.findall(r"#define (MCORB_BOW_[A-Z_]+) (\d+)", src))
    assert defs["MCORB_BOW_TRANSFORM"] == "1" and defs["MCORB_BOW_MATCH"] == "2"
    kcap_4000 = (4000 + 4 * 8 + 48 + 63) // 64 * 64      # mcorb_rig_kcap at nfeatures = 4000, 8 levels
    assert int(defs["MCORB_BOW_MAX_KCAP"]) >= kcap_4000
    assert (pkg._lib.BOW_TRANSFORM, pkg._lib.BOW_MATCH) == (1, 2)


def test_python_and_adapter_mirrors_exist():
    assert callable(getattr(pkg.Rig, "set_vocabulary")) and callable(getattr(pkg.Rig, "bow_tracks"))
    assert callable(getattr(pkg.MultiCameraFrame, "setVocabulary"))
    hpp = open(os.path.join(ROOT, "include", "mcorb_adapter.hpp")).read()
    assert "void setVocabulary(const ORBVocabulary *voc" in hpp and "BoW_vecs" in hpp and "BoW_feats" in hpp
