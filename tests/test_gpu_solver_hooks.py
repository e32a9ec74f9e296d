"""The five minimal solvers on the device at chosen problems: mcorb_dev_sac_solve_selftest, mcorb_dev_sac_solve_rig_selftest,
mcorb_dev_rel_solve_selftest, mcorb_dev_ess_solve_selftest and mcorb_dev_align_solve_selftest against the host hooks on the tables
of solver_hook_cases.py.  Every comparison is floats as raw bytes, no tolerance, no excluded row: the host side's accuracy is held
by the CPU files at their stated marks, and equality carries those marks to the device.

The self-test kernels run the text the estimators' hypotheses kernels run behind the sample -- k_ess_hypotheses' ess_group_models
with its sixteen lanes and shared EssGroup, k_sac_hypotheses_rig's sac_rig_quad with its shuffles and writer rule, the header
functions of the other three -- in the estimators' launch shapes, one launch a table.

On the commit before these entries existed every test of this file fails (`python -m pytest -m gpu
tests/test_gpu_solver_hooks.py`): the package has no dev_ess_solve."""
import numpy as np
import pytest

import align_cases as AC
import align_ref as AR
import ess_cases as EC
import ess_ref as ER
import kfdb_cases as K
import pose_cases as PC
import rel_cases as RC
import rel_ref as RR
import sac_cases as SC
import sac_ref as S
import sac_rig_cases as SRC
import sac_rig_ref as SR
import solver_hook_cases as H

pytestmark = pytest.mark.gpu
NAMES = sorted(H.SOLVERS)


@pytest.fixture(scope="module")
def mc():
    import mcorb
    assert hasattr(mcorb, "dev_ess_solve")
    return mcorb


@pytest.fixture(scope="module")
def lm(mc):
    return mc.LocalMap(mc.ORBVocabulary().create(**K.vocabulary()), device=0, max_landmarks=4096, max_candidates=1024)


_FIRST = {}


def first_run(mc, solver):
    """-> (the table, the host hook's result, one call a problem; the device's, one launch): computed once, never changed"""
    if solver not in _FIRST:
        table, host, dev = H.SOLVERS[solver]
        rows = table()
        _FIRST[solver] = (rows, host(mc, rows), dev(mc, rows))
    return _FIRST[solver]


def differing(rows, a, b):
    bad = H.same(a, b)
    return [rows[i][0] for i in bad[:8]], len(bad)


@pytest.mark.parametrize("solver", NAMES)
def test_device_equals_host_hook(mc, solver):
    """the whole table in one launch: the count and every model slot of every problem -- R, t, E, z, the gap, the valid flag, the
    rig's mask, winner and winning pose"""
    rows, host, dev = first_run(mc, solver)
    print("%s: %d problems, %d of them hostile, counts %s" % (solver, len(rows), sum(1 for r in rows if r[1]), np.bincount(host[0]).tolist()))
    assert differing(rows, host, dev) == ([], 0)


@pytest.mark.parametrize("solver", NAMES)
def test_launch_shape_edges(mc, solver):
    """tables cut to either side of an EssGroup workgroup (4 problems), a wave of quads (16), a wave of lanes (64) and several
    workgroups, hostile and well-posed rows alternating"""
    rows, host, dev = first_run(mc, solver)
    order = H.mixed(rows)
    for n in H.CUTS:
        idx = order[:n]
        got = H.SOLVERS[solver][2](mc, [rows[i] for i in idx])
        assert differing([rows[i] for i in idx], H.take(host, idx), got) == ([], 0), n


@pytest.mark.parametrize("solver", NAMES)
def test_neighbours_do_not_matter(mc, solver):
    """the full table reversed, and with the hostile rows interleaved one for one with well-posed ones: every problem's bytes are
    those of the first run -- an EssGroup indexed by the wrong group, a barrier that a NaN group skips or a shuffle that leaves
    its quad would show here"""
    rows, host, dev = first_run(mc, solver)
    for what, idx in (("reversed", list(range(len(rows)))[::-1]), ("interleaved", H.mixed(rows))):
        got = H.SOLVERS[solver][2](mc, [rows[i] for i in idx])
        assert differing([rows[i] for i in idx], H.take(dev, idx), got) == ([], 0), what


def test_which_roots_were_kept(mc):
    """on the hypotheses with a rejected root between two kept ones the device's z list is the host's, not only its length, and
    the E slots lie in ascending z"""
    rows, host, dev = first_run(mc, "ess")
    at = {r[0]: i for i, r in enumerate(rows)}
    assert len(H.ESS_BETWEEN) >= 36
    for name, pattern in H.ESS_BETWEEN:
        i = at[name]
        k = int(dev[0][i])
        assert k == pattern.count("1") == int(host[0][i]), name
        assert dev[2][i].tobytes() == host[2][i].tobytes(), name
        z = dev[2][i][:k].tolist()
        assert z == sorted(z) and len(set(z)) == k, name
        assert dev[1][i].tobytes() == host[1][i].tobytes() and not dev[1][i][k:].any() and dev[1][i][:k].any(axis=1).all(), name
    # everywhere: the roots ascend, and what lies behind the count is zero
    for i in range(len(rows)):
        k = int(dev[0][i])
        z = dev[2][i][:k].tolist()
        assert z == sorted(z) and not dev[2][i][k:].any() and not dev[1][i][k:].any(), rows[i][0]


# ---------------------------------------------------------------------------------------------------------------------------
# the production path: every hypothesis's sample of a seeded scene cut into a problem
# ---------------------------------------------------------------------------------------------------------------------------
def test_essential_pose_slots_are_the_selftests_models(mc, lm):
    """every slot's E of every hypothesis (last_essential_counts) is the self-test's model of that hypothesis's sample"""
    its = 257
    truth, matches, moved = EC.scene("general", n=200, seed=EC.first_seed("general", 0.1), noise=0.1)
    got = EC.run(mc, lm, matches, max_iterations=its, seed=5)
    assert got.status == ER.OK
    count, valid, models = lm.last_essential_counts()
    rows = [("h %d" % h, True, [tuple(float(w) for w in matches[i]) for i in ER.sample(5, h, len(matches))[0]]) for h in range(its)]
    assert list(got.sample) == ER.sample(5, got.best_hypothesis, len(matches))[0]
    n, E, z = H.dev_ess(mc, rows)
    assert E.tobytes() == models.tobytes()
    assert valid.reshape(its, 10).sum(axis=1).tolist() == n.tolist()
    assert E[got.best_hypothesis, got.best_root].tobytes() == got.E.tobytes()


def by_the_headers_rule(mc, view, poses, fourth):
    """sac_root_beats over a list of poses: the smallest score at the fourth observation, a tie to the first, a NaN never"""
    best, best_score = None, None
    for R, t in poses:
        sc = float(mc.sac_eval(view, R, t, [fourth[0]], [[fourth[1], fourth[2]]], [fourth[4]])[0])
        if sc == sc and (best is None or sc < best_score):
            best, best_score = (R, t), sc
    return best


@pytest.mark.parametrize("solver", ["central", "rig"])
def test_ransac_pose_winner_is_the_selftests_model(mc, lm, solver):
    """the winner's pose is, of the self-test's list on the winner's sample, the one the header's rule picks at the fourth
    observation; with the rig solver it is also the pose the self-test's own writer lane left"""
    cams, truth, obs, match, moved = SC.scene(4, nlm=200, seed=3)
    got = SRC.run(mc, lm, cams, obs, solver, match=match, max_iterations=257, seed=9)
    assert got.status == S.OK and got.best_hypothesis >= 0
    four = [obs[i] for i in got.sample]
    view = H.view_of(mc, cams)
    if solver == "central":
        assert len(set(o[0] for o in four)) == 1
        n, R, t = H.dev_sac(mc, [("winner", True, cams, four[0][0], [[o[1], o[2]] for o in four[:3]], [list(o[4]) for o in four[:3]])])
    else:
        n, R, t, mask, best, Rb, tb = H.dev_rig(mc, [("winner", True, cams, [o[0] for o in four], [[o[1], o[2]] for o in four], [list(o[4]) for o in four])])
        assert best[0] >= 0 and Rb[0].tobytes() == got.sac_R.tobytes() and tb[0].tobytes() == got.sac_t.tobytes()
    pick = by_the_headers_rule(mc, view, [(R[0, k], t[0, k]) for k in range(int(n[0]))], four[3])
    assert pick is not None and pick[0].tobytes() == got.sac_R.tobytes() and pick[1].tobytes() == got.sac_t.tobytes()


def test_relative_pose_winner_is_the_selftests_model(mc, lm):
    cams, truth, matches, moved = RC.scene(8, 200, RC.first_seed())
    got = RC.run(mc, lm, cams, matches, max_iterations=257, seed=4)
    assert got.status == RR.OK and list(got.sample) == RR.sample(4, got.best_hypothesis, len(matches))[0]
    n, R, t = H.dev_rel(mc, [("winner", True, cams, [matches[i] for i in got.sample])])
    assert n[0] == 1 and R[0].tobytes() == got.R.tobytes() and t[0].tobytes() == got.t.tobytes()


def test_align_pose_winner_and_fit_are_the_selftests_models(mc, lm):
    """mode sac: the winning hypothesis's pose is the self-test's on its three pairs; mode all: the answer is the self-test's over
    all pairs"""
    truth, p1, p2, moved = AC.scene(n=257, seed=AC.first_seed(n=257))
    got = AC.run(mc, lm, p1, p2, mode=AR.SAC, max_iterations=257, seed=6)
    assert got.status == AR.OK and list(got.sample) == AR.sample(6, got.best_hypothesis, len(p1))[0]
    smp = list(got.sample)
    everything = AC.run(mc, lm, p1, p2, mode=AR.ALL)
    valid, R, t, gap = H.dev_align(mc, [("winner", True, p1[smp], p2[smp], None), ("all", True, p1, p2, None)])
    assert valid.tolist() == [1, 1]
    assert R[0].tobytes() == got.sac_R.tobytes() and t[0].tobytes() == got.sac_t.tobytes()
    assert R[1].tobytes() == everything.R.tobytes() and t[1].tobytes() == everything.t.tobytes()


# ---------------------------------------------------------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------------------------------------------------------
def test_refusals_and_empty_tables(mc):
    """n == 0 launches nothing; a camera index outside the rig and a null pointer are refused as the host hooks refuse them, before
    anything is queued; a valid call right behind a refused one gives the first run's bytes"""
    L = mc._lib.load()
    for solver in NAMES:
        rows, host, dev = first_run(mc, solver)
        empty = H.SOLVERS[solver][2](mc, [])
        assert all(len(a) == 0 for a in empty), solver
    rows, host, dev = first_run(mc, "rig")
    ok = [rows[i] for i in H.mixed(rows)[:5]]
    assert len(ok[3][2]) == 1 and len(ok[0][2]) > 1      # (index 1: inside the table's ncams, outside the problem's own rig)
    for bad in (-1, 1, 4, 16):
        broken = list(ok)
        broken[3] = broken[3][:3] + ([0, bad, 0, 0],) + broken[3][4:]
        with pytest.raises(mc.McorbError) as e:
            H.dev_rig(mc, broken)
        assert e.value.code == mc.E_ARG and "a camera index outside the rig" in str(e.value)
        assert H.same(H.dev_rig(mc, ok), H.take(dev, H.mixed(rows)[:5])) == []
    rows, host, dev = first_run(mc, "rel")
    ok = [rows[i] for i in H.mixed(rows)[:5]]
    broken = list(ok)
    broken[4] = broken[4][:3] + ([(99,) + tuple(m[1:]) for m in broken[4][3]],)
    with pytest.raises(mc.McorbError) as e:
        H.dev_rel(mc, broken)
    assert e.value.code == mc.E_ARG
    assert H.same(H.dev_rel(mc, ok), H.take(dev, H.mixed(rows)[:5])) == []
    # a rig of one camera beside rigs of eight: index 1 lies inside the table's ncams and outside the problem's own rig
    small = [r for r in rows if r[0] == "a rig of one camera, outward, 0"][0]
    assert len(small[2]) == 1 and len(ok[1][2]) > 1
    with pytest.raises(mc.McorbError) as e:
        H.dev_rel(mc, [ok[1], small[:3] + ([(1,) + tuple(m[1:]) for m in small[3]],)])
    assert e.value.code == mc.E_ARG and "a camera index outside the rig" in str(e.value)
    assert H.same(H.dev_rel(mc, ok), H.take(dev, H.mixed(rows)[:5])) == []
    # the entries themselves: a null pointer in each, ncams and a camera index out of range in the two that take a rig
    one = np.zeros(17 * 16)
    cnt = np.zeros(17 * 4, np.int32)
    o, c = one.ctypes.data, cnt.ctypes.data
    rig = lambda ncams, cams, cam: L.mcorb_dev_sac_solve_rig_selftest(0, 1, ncams, cams, cam, o, o, c, o, o, c, c, o, o)   # noqa: E731
    rel = lambda ncams, cams, cam2: L.mcorb_dev_rel_solve_selftest(0, 1, ncams, cams, c, o, cam2, o, c, o, o)            # noqa: E731
    for call in (rig, rel):
        assert call(1, None, c) == mc.E_ARG and call(1, o, None) == mc.E_ARG
        assert call(0, o, c) == mc.E_ARG and call(mc._lib.MAX_CAMS + 1, o, c) == mc.E_ARG
        bad = np.zeros(17 * 4, np.int32)
        bad[3] = 1
        assert call(1, o, bad.ctypes.data) == mc.E_ARG and b"a camera index outside the rig" in L.mcorb_last_error()
        bad[3] = -1
        assert call(1, o, bad.ctypes.data) == mc.E_ARG
    assert L.mcorb_dev_sac_solve_rig_selftest(0, -1, 1, o, c, o, o, c, o, o, c, c, o, o) == mc.E_ARG
    assert L.mcorb_dev_rel_solve_selftest(0, -1, 1, o, c, o, c, o, c, o, o) == mc.E_ARG
    assert H.same(H.dev_rel(mc, ok), H.take(dev, H.mixed(rows)[:5])) == []
    assert L.mcorb_dev_ess_solve_selftest(0, 1, None, one.ctypes.data, one.ctypes.data, cnt.ctypes.data, one.ctypes.data, one.ctypes.data) == mc.E_ARG
    assert L.mcorb_dev_sac_solve_selftest(0, 1, one.ctypes.data, None, one.ctypes.data, cnt.ctypes.data, one.ctypes.data, one.ctypes.data) == mc.E_ARG
    assert L.mcorb_dev_align_solve_selftest(0, 1, None, one.ctypes.data, one.ctypes.data, one.ctypes.data, cnt.ctypes.data, one.ctypes.data,
                                            one.ctypes.data, one.ctypes.data) == mc.E_ARG
    assert L.mcorb_dev_align_solve_selftest(0, -1, cnt.ctypes.data, one.ctypes.data, one.ctypes.data, one.ctypes.data, cnt.ctypes.data,
                                            one.ctypes.data, one.ctypes.data, one.ctypes.data) == mc.E_ARG
    rows, host, dev = first_run(mc, "ess")
    assert H.same(H.dev_ess(mc, rows[:5]), H.take(dev, list(range(5)))) == []
