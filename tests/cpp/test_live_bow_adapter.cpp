// include/mcorb_adapter.hpp's bound vocabulary, driven as MC-SLAM would: setVocabulary once at init, then setData +
// extractFeaturesParallel, which fills BoW_vecs / BoW_feats, and the BoW-guided computeIntraMatches, which reads the job's tracks.
// Both must equal an unbound front end's explicit transform / computeIntraMatches of the same frame.
//   test_live_bow_adapter C W H N FRAME VOCABULARY_TEXT_FILE
#include <stdio.h>
#include <stdlib.h>

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
        mcorb::MultiCameraFrontEnd bound(C, W, H, p), plain(C, W, H, p);
        bound.setVocabulary(&voc, 4);
        std::vector<std::vector<uint8_t>> imgs(C, std::vector<uint8_t>((size_t)W * H));
        std::vector<const uint8_t *> ptrs;
        for (int c = 0; c < C; c++) {
            mcorb_synth_rig_frame(frame, C, c, W, H, imgs[c].data(), W);
            ptrs.push_back(imgs[c].data());
        }
        for (mcorb::MultiCameraFrontEnd *fe : {&bound, &plain}) {
            fe->setData(ptrs, W);
            fe->extractFeaturesParallel();
        }
        if ((int)bound.BoW_vecs.size() != C || (int)bound.BoW_feats.size() != C || !plain.BoW_vecs.empty()) {
            fprintf(stderr, "BoW_vecs / BoW_feats not filled as expected\n");
            return 1;
        }
        for (int c = 0; c < C; c++) {
            mcorb::ORBVocabulary::BowVector bv;
            mcorb::ORBVocabulary::FeatureVector fv;
            plain.transform(c, voc, bv, fv, 4);
            if (bv != bound.BoW_vecs[c] || fv != bound.BoW_feats[c] || bv.size() < 100) {
                fprintf(stderr, "camera %d: BoW vectors differ (%zu / %zu words)\n", c, bv.size(), bound.BoW_vecs[c].size());
                return 1;
            }
        }
        std::vector<mcorb::IntraMatch> mb, mp;
        std::vector<unsigned int> wb, wp;
        bound.computeIntraMatches(mb, wb, voc);
        plain.computeIntraMatches(mp, wp, voc);
        if (mb.size() != mp.size() || wb != wp || mb.size() < 50) {
            fprintf(stderr, "tracks differ: %zu / %zu\n", mb.size(), mp.size());
            return 1;
        }
        for (size_t m = 0; m < mb.size(); m++)
            if (mb[m].matchIndex != mp[m].matchIndex || mb[m].n_rays != mp[m].n_rays) { fprintf(stderr, "track %zu differs\n", m); return 1; }
        printf("tracks %zu, words %zu\n", mb.size(), wb.size());
    } catch (const std::exception &e) {
        fprintf(stderr, "%s\n", e.what());
        return 1;
    }
    return 0;
}
