// mc-slam_amd/csrc/mcorb_triangulate.h built by plain g++ -ffp-contract=off, no HIP: reads problems from IN (int32 n, int32 nv[n],
// then per problem 2 nv + 12 nv doubles) and writes per problem X[3] doubles and the solver's branch (int32) to OUT.
//   test_triangulate IN OUT
#include <stdio.h>

#include <vector>

#include "mcorb_triangulate.h"

int main(int argc, char **argv)
{
    if (argc != 3) { fprintf(stderr, "usage: %s IN OUT\n", argv[0]); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    int n = 0;
    if (fread(&n, 4, 1, f) != 1 || n < 0) return 2;
    std::vector<int> nv(n);
    if (fread(nv.data(), 4, n, f) != (size_t)n) return 2;
    FILE *o = fopen(argv[2], "wb");
    if (!o) return 2;
    for (int i = 0; i < n; i++) {
        if (nv[i] < 2 || nv[i] > MCORB_MAX_CAMS) return 2;
        double x[2 * MCORB_MAX_CAMS], P[12 * MCORB_MAX_CAMS], X[3];
        if (fread(x, 8, 2 * nv[i], f) != (size_t)(2 * nv[i]) || fread(P, 8, 12 * nv[i], f) != (size_t)(12 * nv[i])) return 2;
        const double *Pp[MCORB_MAX_CAMS];
        for (int v = 0; v < nv[i]; v++) Pp[v] = P + 12 * v;
        const int br = mcorb::triangulate(x, Pp, nv[i], X);
        fwrite(X, 8, 3, o);
        fwrite(&br, 4, 1, o);
    }
    fclose(o);
    fclose(f);
    return 0;
}
