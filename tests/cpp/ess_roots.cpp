// ess_roots.cpp -- which real roots of each hypothesis' degree-10 polynomial give a model (csrc/mcorb_ess.h: ess_solve5's steps, one
// by one), as a stand-alone program built by tests/test_hostile_cpu.py.  The ten slots of a hypothesis hold its models compacted, so
// the read-back cannot say whether a rejected root lay between two kept ones: this can.  argv[1]: test_ess_sanitize.cpp's input
// file.  Prints one line per hypothesis: its index and one character per real root in ascending order, 1 kept, 0 rejected ("-"
// without a root or without a sample).
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../include/mcorb.h"
#include "mcorb_ess.h"

using namespace mcorb;

int main(int argc, char **argv)
{
    if (argc != 2) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    int32_t head[2];
    double par[7];
    uint64_t seed;
    int bad = 0;
    bad += fread(head, sizeof(head), 1, f) != 1;
    bad += fread(par, sizeof(par), 1, f) != 1;
    bad += fread(&seed, sizeof(seed), 1, f) != 1;
    const int n = head[0], H = head[1];
    std::vector<EssObs> obs((size_t)n);
    bad += fread(obs.data(), sizeof(EssObs), (size_t)n, f) != (size_t)n;
    fclose(f);
    if (bad) return 2;

    EssJob job;
    memset(&job, 0, sizeof(job));
    job.fx = par[0], job.fy = par[1], job.s = par[2], job.u0 = par[3], job.v0 = par[4];
    job.seed = seed;
    job.S = n;
    job.H = H;
    for (int h = 0; h < H; h++) {
        double d1[kEssSample][3], d2[kEssSample][3], B[36], table[200], det[kEssNodes], p[kEssNodes], roots[kEssRoots], E[9];
        int32_t smp[kEssSample];
        printf("%d ", h);
        int nr = 0;
        if (ess_sample(job, h, obs.data(), smp, d1, d2)) {
            ess_basis(d1, d2, B);
            for (int k = 0; k < 10; k++) ess_cubic(B, k, table + 20 * k);
            for (int k = 0; k < kEssNodes; k++) det[k] = ess_det_at(table, k, 1.0);
            for (int j = 0; j < kEssNodes; j++) p[j] = ess_coefficient(det, j);
            const double rho = ess_scale(p);
            for (int k = 0; k < kEssNodes; k++) det[k] = ess_det_at(table, k, rho);
            for (int j = 0; j < kEssNodes; j++) p[j] = ess_coefficient(det, j);
            nr = ess_real_roots(p, roots);
            for (int r = 0; r < nr; r++) putchar(ess_root_model(table, B, d1, d2, rho * roots[r], E) ? '1' : '0');
        }
        printf(nr ? "\n" : "-\n");
    }
    return 0;
}
