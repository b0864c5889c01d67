// Host-only: which plans the LDS Cholesky kernel serves (vjf_chol_lds_ok) with 33-float block rows and 32 control floats,
// against the predicate as it stood with 1024-float blocks and 192 control floats.  Every n % 4 == 0, n <= 224, dz <= 32.
//   hipcc --offload-arch=gfx950 -O1 -o tools/chol_lds_plans tools/chol_lds_plans.hip && tools/chol_lds_plans
// Exit status 1 if a plan that was served is refused now.
#include <cstdio>
#include "../vjf_amd/csrc/vjf_chol_kernel.h"

static size_t old_bytes(int n, int dz) {
    const int nbl = (n + 31) / 32, dzp = vjf_chol_dzp(dz);
    return ((size_t)(nbl * (nbl + 1) / 2 + nbl) * 1024 + (size_t)nbl * 32 * dzp * (dzp <= 16 ? 1 : 2) + 192) * 4;
}
int main() {
    const size_t bound = 160 * 1024 - 512;
    int served_old = 0, served_new = 0, lost = 0, gained = 0;
    size_t max_new = 0;
    for (int n = 4; n <= 224; n += 4)
        for (int dz = 1; dz <= 32; ++dz) {
            VjfPlan P{};
            P.n = n; P.dz = dz;
            const bool o = old_bytes(n, dz) <= bound, w = vjf_chol_lds_ok(P);
            served_old += o; served_new += w; lost += o && !w; gained += !o && w;
            if (w && vjf_chol_lds_bytes(P) > max_new) max_new = vjf_chol_lds_bytes(P);
            if (o != w) printf("n=%d dz=%d: old %zu B (%s) new %zu B (%s)\n", n, dz, old_bytes(n, dz), o ? "ok" : "no", vjf_chol_lds_bytes(P), w ? "ok" : "no");
        }
    printf("plans n %% 4 == 0, n <= 224, dz <= 32: served before %d, now %d; lost %d, gained %d; bound %zu B, largest served now %zu B\n",
           served_old, served_new, lost, gained, bound, max_new);
    for (int nbl = 1; nbl <= 7; ++nbl)
        for (int dz : {16, 32}) {
            VjfPlan P{};
            P.n = 32 * nbl; P.dz = dz;
            printf("  nbl=%d dzp=%d: %zu -> %zu B%s\n", nbl, dz, old_bytes(P.n, dz), vjf_chol_lds_bytes(P), vjf_chol_lds_ok(P) ? "" : "  (refused)");
        }
    return lost ? 1 : 0;
}
