// Host-side plan helpers of the weight-gradient launcher (plain C++: scripts/wgrad_plan_check.cpp compiles them alone, with sanitizers).
#pragma once

// wgrad_flat_kernel's LDS-DMA form lands the next tile's input row in the ring slot of the tap row a column block does not read: it needs every
// column block (64 * ntw columns n = tap * CW + c of a chunk of CW channels) to read at most two of the three tap rows r = n / (3 CW) -- the
// blocks of the full chunks and of the shorter last one.  Narrow chunks (a block of 320 columns spans all nine taps of 36 channels) do not.
inline bool flat_dma_fits(int Cin, int cw, int nnb, int ntw) {
    const int nch = (Cin + cw - 1) / cw;
    const int widths[2] = {nch > 1 ? cw : Cin, Cin - (nch - 1) * cw};
    for (int CW : widths)
        for (int nb = 0; nb < nnb; ++nb) {
            const int lo = nb * 64 * ntw;
            int hi = lo + 64 * ntw;
            if (hi > 9 * CW) hi = 9 * CW;
            if (lo >= hi) continue;             // spare columns only
            if ((hi - 1) / (3 * CW) - lo / (3 * CW) > 1) return false;
        }
    return true;
}
