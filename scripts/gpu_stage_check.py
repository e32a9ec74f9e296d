"""Stage-by-stage GPU-vs-oracle comparison (development aid; the real tests live in tests/)."""
import sys, os, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import numpy as np
import mcorb
import oracle_lib as O
import stage_cases as S

W, H, C, N = (int(a) for a in (sys.argv[1:5] + ["1280", "720", "4", "2000"][len(sys.argv) - 1:]))
imgs = [mcorb.synth_rig_frame(0, C, c, W, H) for c in range(C)]
rig = mcorb.Rig(C, W, H, 1, 1, nfeatures=N)
rig.upload(imgs)
t = time.time(); rig.extract(C); print("extract ms", (time.time() - t) * 1e3, rig.timing())
t = time.time(); rig.extract(C); print("extract ms (2nd)", (time.time() - t) * 1e3, rig.timing())
ex = O.OracleExtractor(N)
ok = True
descs = []
for c in range(C):
    exp = S.oracle_stages(ex, imgs[c])          # the comparison of tests/test_gpu_stages.py: first differing element per stage
    diffs = S.diff_image(rig, c, exp)
    for d in diffs:
        print("cam", c, d)
    descs.append(exp["desc"])
    print("cam", c, "n", len(exp["kps"]), "mono", exp["mono"], "stages equal" if not diffs else "%d stages differ" % len(diffs))
    ok &= not diffs
t = time.time(); rig.match(1); print("match ms", (time.time() - t) * 1e3, rig.timing())
for i in range(C - 1):
    for j in range(i + 1, C):
        gi, gd = rig.pair_knn2(0, i, j); oi, od = O.knn2(descs[i], descs[j])
        s = np.array_equal(gi, oi) and np.array_equal(gd, od)
        g1, g2 = rig.pair_matches(0, i, j); o1, o2 = O.bruteforce_match(descs[i], descs[j])
        s2 = np.array_equal(g1, o1) and np.array_equal(g2, o2)
        print("pair", i, j, "knn2", s, "matches", s2, len(g1))
        ok &= s and s2
tr, mg = rig.tracks(0); otr, omg = O.intra_matches(descs)
print("tracks", tr.shape, otr.shape, np.array_equal(tr, otr), mg, omg)
ok &= np.array_equal(tr, otr) and mg == omg
print("ALL OK" if ok else "MISMATCH")
sys.exit(0 if ok else 1)
