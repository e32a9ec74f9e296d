// include/mcorb_adapter.hpp's LF binding, driven as MC-SLAM would: setVocabulary and setLfConfig once at init, then setData +
// extractFeaturesParallel, which fills intraMatches / intramatch_size / mono_size / lfBoW / lfFeatVec.  They must equal the
// explicit C-ABI chain on the same frame: mcorb_rig_obtain_lf_features on the job's BoW-guided tracks with words_ all 1, and the
// vocabulary's transform of the returned descriptors.
//   test_live_lf_adapter C W H N FRAME VOCABULARY_TEXT_FILE
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>

#include "mcorb_adapter.hpp"

int main(int argc, char **argv)
{
    if (argc != 7) { fprintf(stderr, "usage: %s C W H N FRAME VOCABULARY\n", argv[0]); return 2; }
    const int C = atoi(argv[1]), W = atoi(argv[2]), H = atoi(argv[3]), N = atoi(argv[4]), frame = atoi(argv[5]);
    try {
        mcorb::ORBVocabulary voc;
        if (!voc.loadFromTextFile(argv[6])) { fprintf(stderr, "cannot load %s\n", argv[6]); return 2; }
        mcorb_params p;
        mcorb_default_params(&p);
        p.nfeatures = N;
        mcorb::MultiCameraFrontEnd fe(C, W, H, p);
        std::vector<std::array<double, 9>> K(C), R(C);
        std::vector<std::array<double, 3>> t(C);
        for (int c = 0; c < C; c++) {   // a rig of parallel cameras on a 0.1 baseline
            K[c] = {0.9 * W, 0.0, W / 2.0, 0.0, 0.9 * W, H / 2.0, 0.0, 0.0, 1.0};
            R[c] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
            t[c] = {-0.1 * c, 0.0, 0.0};
        }
        fe.setVocabulary(&voc, 4);
        fe.setLfConfig(K, R, t, 3000);
        std::vector<std::vector<uint8_t>> imgs(C, std::vector<uint8_t>((size_t)W * H));
        std::vector<const uint8_t *> ptrs;
        for (int c = 0; c < C; c++) {
            mcorb_synth_rig_frame(frame, C, c, W, H, imgs[c].data(), W);
            ptrs.push_back(imgs[c].data());
        }
        fe.setData(ptrs, W);
        fe.extractFeaturesParallel();
        const int n = (int)fe.intraMatches.size();
        if (n < 100 || fe.intramatch_size + fe.mono_size != n || fe.lfBoW.empty()) {
            fprintf(stderr, "LF outputs not filled: %d features, %d + %d, %zu words\n", n, fe.intramatch_size, fe.mono_size, fe.lfBoW.size());
            return 1;
        }
        // the explicit chain on the job's own tracks
        mcorb_rig *r = fe.rig();
        const int cap = 1 << 16;
        std::vector<int32_t> tr((size_t)cap * C), rays(cap);
        std::vector<uint32_t> w(cap);
        int nt = 0, nw = 0;
        if (mcorb_rig_get_bow_tracks(r, 0, 0, tr.data(), rays.data(), cap, &nt, w.data(), cap, &nw) != MCORB_OK) { fprintf(stderr, "bow tracks\n"); return 1; }
        std::vector<uint32_t> ones((size_t)nt + 1, 1u);
        std::vector<mcorb_camera> cams(C);
        for (int c = 0; c < C; c++) {
            memcpy(cams[c].K, K[c].data(), sizeof(cams[c].K));
            for (int i = 0; i < 3; i++) {
                for (int k = 0; k < 3; k++) cams[c].Rt[4 * i + k] = R[c][3 * i + k];
                cams[c].Rt[4 * i + 3] = t[c][i];
            }
        }
        std::vector<mcorb_lf_feature> ex((size_t)std::max(3000, nt) + 1);
        std::vector<uint32_t> wf((size_t)nt + 1);
        int ne = 0, ni = 0, nm = 0, nwf = 0;
        if (mcorb_rig_obtain_lf_features(r, 0, 0, tr.data(), nt, ones.data(), cams.data(), nullptr, 0, nullptr, 3000, ex.data(), (int)ex.size(),
                                         &ne, &ni, &nm, wf.data(), (int)wf.size(), &nwf) != MCORB_OK) {
            fprintf(stderr, "obtain_lf_features: %s\n", mcorb_last_error());
            return 1;
        }
        if (ne != n || ni != fe.intramatch_size || nm != fe.mono_size) { fprintf(stderr, "counts differ: %d / %d\n", ne, n); return 1; }
        std::vector<uint8_t> descs((size_t)n * 32);
        for (int i = 0; i < n; i++) {
            const mcorb::IntraMatch &m = fe.intraMatches[i];
            bool same = m.mono == (ex[i].mono != 0) && m.n_rays == ex[i].n_rays && memcmp(m.matchDesc.data(), ex[i].desc, 32) == 0 &&
                        memcmp(m.point3D.data(), ex[i].point3d, 24) == 0 && memcmp(m.uv_ref.data(), ex[i].uv_ref, 8) == 0;
            for (int c = 0; c < MCORB_MAX_CAMS; c++) same = same && m.matchIndex[c] == ex[i].match_index[c];
            if (!same) { fprintf(stderr, "feature %d differs\n", i); return 1; }
            memcpy(descs.data() + (size_t)i * 32, ex[i].desc, 32);
        }
        mcorb::ORBVocabulary::BowVector bv;
        mcorb::ORBVocabulary::FeatureVector fv;
        voc.transform(descs.data(), n, bv, fv, 4);
        if (bv != fe.lfBoW || fv != fe.lfFeatVec) { fprintf(stderr, "lfBoW / lfFeatVec differ\n"); return 1; }
        printf("lf features %d (%d tracks, %d mono), words %zu\n", n, fe.intramatch_size, fe.mono_size, bv.size());
    } catch (const std::exception &e) {
        fprintf(stderr, "%s\n", e.what());
        return 1;
    }
    return 0;
}
