// The index maps of the one-wave 1024-point transform's two exchanges, one-piece and in halves (libredio_amd/csrc/fft_core.h:
// fft1kn_x1_*, fft1kn_x2_*, fft1kn_x1h_*, fft1kn_x2h_*), as tables for tests/test_emu_chain_block_schedule.py.  Tests only.
#include "../../libredio_amd/csrc/fft_core.h"

using namespace redio;

extern "C" {

// v[0..4] = FFT1KN_ROW1, FFT1KN_ROW2, FFT1KN_LDS, FFT1KN_HROW1, FFT1KN_HALF_LDS
void emu_sched_consts(int *v)
{
    v[0] = FFT1KN_ROW1; v[1] = FFT1KN_ROW2; v[2] = FFT1KN_LDS; v[3] = FFT1KN_HROW1; v[4] = FFT1KN_HALF_LDS;
}

// exchange x (1 or 2), tables of [64 lanes][16 elements]: the one-piece store and load index; the half each store / load belongs
// to and its index within the half.  Element order of a lane: X1 store 4 k4 + d0, X1 load e, X2 store k2 + 4 k3, X2 load f --
// the register index the kernel uses on either side.
int emu_sched_maps(int x, int *store1, int *load1, int *store_half, int *store_h, int *load_half, int *load_h)
{
    if (x != 1 && x != 2) return 1;
    for (int lane = 0; lane < 64; ++lane)
        for (int i = 0; i < 16; ++i) {
            const int o = 16 * lane + i;
            if (x == 1) {
                store1[o] = fft1kn_x1_store(lane, i >> 2, i & 3);
                load1[o] = fft1kn_x1_load(lane, i);
                store_half[o] = fft1kn_x1h_store_half(lane);
                store_h[o] = fft1kn_x1h_store(lane, i >> 2, i & 3);
                load_half[o] = fft1kn_x1h_load_half(i);
                load_h[o] = fft1kn_x1h_load(lane, i);
            } else {
                store1[o] = fft1kn_x2_store(lane, i & 3, i >> 2);
                load1[o] = fft1kn_x2_load(lane, i);
                store_half[o] = fft1kn_x2h_store_half(lane);
                store_h[o] = fft1kn_x2h_store(lane, i & 3, i >> 2);
                load_half[o] = fft1kn_x2h_load_half(i);
                load_h[o] = fft1kn_x2h_load(lane, i);
            }
        }
    return 0;
}

// one-piece index i of exchange x -> (half, index within the half)
int emu_sched_half_of(int x, int i, int *half)
{
    return x == 1 ? fft1kn_x1_half_of(i, half) : fft1kn_x2_half_of(i, half);
}

}
