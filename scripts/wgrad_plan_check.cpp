// Stand-alone check of the host-side plan helper flat_dma_fits (unet_amd/csrc/wgrad_plan.h) against a brute-force count of the tap rows
// every column block reads, over every input-channel count up to 1200 and both column-tile counts; meant to run under sanitizers:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I unet_amd/csrc scripts/wgrad_plan_check.cpp -o /tmp/wgrad_plan_check && /tmp/wgrad_plan_check
#include <cstdio>
#include <initializer_list>

#include "wgrad_plan.h"

int main() {
    long n = 0, yes = 0;
    for (int ntw : {5, 7})
        for (int Cin = 1; Cin <= 1200; ++Cin) {
            // chunk width and column blocks as make_wplan derives them
            const int nch = (Cin + 111) / 112;
            const int cw = (((Cin + nch - 1) / nch) + 3) / 4 * 4;
            const int nnb = (((9 * cw + 15) / 16) + 4 * ntw - 1) / (4 * ntw);
            bool want = true;
            const int chunks = (Cin + cw - 1) / cw;
            for (int ch = 0; ch < chunks; ++ch) {
                const int CW = Cin - ch * cw < cw ? Cin - ch * cw : cw;
                for (int nb = 0; nb < nnb; ++nb) {
                    bool rows[3] = {false, false, false};
                    for (int c = nb * 64 * ntw; c < (nb + 1) * 64 * ntw && c < 9 * CW; ++c) rows[(c / CW) / 3] = true;
                    if (rows[0] && rows[1] && rows[2]) want = false;
                }
            }
            const bool got = flat_dma_fits(Cin, cw, nnb, ntw);
            if (got != want) { printf("Cin %d, %d column tiles per wave: flat_dma_fits says %d, the count %d\n", Cin, ntw, got, want); return 1; }
            ++n; yes += got;
        }
    // the shapes the tests and the network use
    struct { int Cin, ntw; bool dma; } known[] = {{9, 5, false}, {36, 5, false}, {36, 7, false}, {96, 7, true}, {100, 5, true}, {112, 5, true},
                                                  {113, 5, false}, {192, 7, true}, {230, 5, true}};
    for (auto& k : known) {
        const int nch = (k.Cin + 111) / 112, cw = (((k.Cin + nch - 1) / nch) + 3) / 4 * 4;
        const int nnb = (((9 * cw + 15) / 16) + 4 * k.ntw - 1) / (4 * k.ntw);
        if (flat_dma_fits(k.Cin, cw, nnb, k.ntw) != k.dma) { printf("Cin %d: expected %d\n", k.Cin, k.dma); return 1; }
    }
    printf("%ld plans checked, %ld take the DMA form\n", n, yes);
    return 0;
}
