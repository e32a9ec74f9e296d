"""The GPU path against the reference's own program text: RECORDED results of the reference binary (tests/golden/ref_*.npz,
never skipping) and, where oracle/_ref/libmcslam_ref_orb.so travelled along, the LIVE binary.  That binary is the reference's
MCSlam/src/ORBextractor.cpp compiled unchanged against the stand-in cv:: types of oracle/refcv.

Pinned by this: the reference's own logic, now for k_select / k_assemble / the cell tables / k_describe_fused / the host stage
directly and not through the oracle.  Not pinned: OpenCV's five primitives (FAST, resize, copyMakeBorder, GaussianBlur,
fastAtan2), which that binary takes from the oracle's restatements (tests/ref_lib.py).  Bit for bit, no tolerance.
Reads oracle/_ref/ and tests/golden/ only."""
import os
import sys

import numpy as np
import pytest

import ref_lib as R

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import make_ref_golden as G  # noqa: E402

pytestmark = pytest.mark.gpu
PATHS = pytest.mark.parametrize("selection,graph", [(2, 0), (2, 1), (1, 0)], ids=["gpu", "gpu-graph", "host"])   # as test_every_path_one_slot


@pytest.fixture(scope="module")
def mc():
    import mcorb
    return mcorb


def _rig(mc, spec, selection, graph, orientation=0):
    kind, C, W, H, frame, (nf, sf, nl, ini, mn), lap = spec
    rig = mc.Rig(C, W, H, 1, 1, nfeatures=nf, scale_factor=sf, nlevels=nl, ini_th_fast=ini, min_th_fast=mn, selection=selection,
                 orientation=orientation)
    rig.set_graph(graph)
    return rig


@PATHS
@pytest.mark.parametrize("name", sorted(G.EXTRACTIONS))
def test_gpu_equals_recorded_reference_extraction(mc, name, selection, graph):
    """three jobs per rig, so that a captured graph is replayed"""
    spec, rec = G.EXTRACTIONS[name], G.load(name)
    C, nl, lap = spec[1], spec[5][2], spec[6]
    imgs = [G.image(spec, c) for c in range(C)]
    for c in range(C):
        assert np.array_equal(G.sha1(imgs[c]), rec["img_sha1_%d" % c]), "the input image is not the recorded one"
    rig = _rig(mc, spec, selection, graph)
    for job in range(3):
        rig.upload(imgs)
        rig.extract(C, lap=lap)
        for c in range(C):
            got = rig.features(c)
            R.same_as_record("%s cam %d job %d" % (name, c, job), rec, c, got, levels=[rig.level(c, l) for l in range(nl)],
                             level_counts=[int((got[1]["octave"] == l).sum()) for l in range(nl)])
    rig.close()


@PATHS
@pytest.mark.parametrize("name", sorted(G.ROTATED))
def test_gpu_equals_recorded_reference_rotated_brief(mc, name, selection, graph):
    """orientation mode: every KeyPoint field but the angle equals the reference's operator(), the angle the reference's IC_Angle,
    the descriptor the reference's computeOrbDescriptor at that angle (staged: the reference itself never calls IC_Angle)"""
    spec, rec = G.ROTATED[name], G.load(name)
    img = G.image(spec, 0)
    assert np.array_equal(G.sha1(img), rec["img_sha1_0"])
    want = R.unpack_keypoints(rec, "kps_0")
    want["angle"] = R.unpack_keypoints(rec, "level_kps")["angle"]
    rig = _rig(mc, spec, selection, graph, orientation=1)
    for job in range(3):
        rig.upload([img])
        rig.extract(1)
        mono, k, d = rig.features(0)
        assert mono == len(want)
        R.same_keypoints("%s job %d, keypoints with IC_Angle (recorded reference)" % (name, job), want, k)
        R.same("%s job %d, computeOrbDescriptor (recorded reference)" % (name, job), rec["desc"], d)
    rig.close()


@pytest.mark.skipif(not R.available(), reason=R.SKIP_REASON)
@pytest.mark.parametrize("W,H,N,frame", [(1280, 720, 2000, 3), (1280, 720, 2000, 12), (1920, 1080, 2000, 3), (1920, 1080, 2000, 12),
                                          (1119, 1118, 2000, 5), (1328, 1223, 2000, 5)])   # the last two: the cell loop's skips (ref_cases.SKIP_EDGE_SIZES)
@pytest.mark.parametrize("orientation", [0, 1])
def test_gpu_equals_live_reference(mc, W, H, N, frame, orientation):
    img = mc.synth_rig_frame(frame, 4, frame % 4, W, H)
    tag = "%dx%d @%d frame %d orientation %d" % (W, H, N, frame, orientation)
    ref = R.RefExtractor(N)
    want = ref(img)                                  # operator(): angle 0
    ext = mc.ORBextractor(N, 1.2, 8, 20, 7, orientation)
    got = ext(img)
    ext.close()
    if orientation == 0:
        R.same_extraction(tag, want, got)
        return
    # mode 1 staged: the reference's IC_Angle on its own pyramid at its own level keypoints, its computeOrbDescriptor at that angle
    lk = ref.compute_keypoints(img)
    ang = [ref.ic_angle(l, lk[l]["x"], lk[l]["y"]) for l in range(8)]
    desc = [ref.orb_descriptor(l, lk[l]["x"], lk[l]["y"], ang[l]) for l in range(8)]
    wk = want[1].copy()
    wk["angle"] = np.concatenate(ang)
    assert want[0] == got[0] == len(wk)
    R.same_keypoints("%s, keypoints with IC_Angle" % tag, wk, got[1])
    R.same("%s, computeOrbDescriptor" % tag, np.concatenate(desc), got[2])
    assert len(wk) > 0.9 * N
