// route_table <nfft> ... : one line "nfft route in_place_ok needs_work" per size, from fft_route() on the stage list that
// redio_fft_create builds (fft_plan_stages).  tests/test_fft_route.py compares the lines with a table written out by hand.
#include "../../libredio_amd/csrc/fft_core.h"
#include "../../libredio_amd/csrc/fft_route.h"
#include <stdio.h>
#include <stdlib.h>

using namespace redio;

static const char *name(FftRoute r)
{
    switch (r) {
    case FFT_ROUTE_WAVE1K: return "wave1k";
    case FFT_ROUTE_P2: return "p2";
    case FFT_ROUTE_64: return "64";
    case FFT_ROUTE_256: return "256";
    case FFT_ROUTE_ONE_WAVE: return "one_wave";
    case FFT_ROUTE_FOUR_WAVE: return "four_wave";
    case FFT_ROUTE_CT: return "ct";
    case FFT_ROUTE_LDS_BATCHED: return "lds_batched";
    case FFT_ROUTE_LDS: return "lds";
    case FFT_ROUTE_MULTIPASS: return "multipass";
    case FFT_ROUTE_TILE_PASSES: return "tile_passes";
    case FFT_ROUTE_GLOBAL: return "global";
    }
    return "?";
}

int main(int argc, char **argv)
{
    for (int i = 1; i < argc; ++i) {
        const int nfft = atoi(argv[i]);
        FftStage st[32];
        const int ns = fft_plan_stages(nfft, st, 32);
        if (ns < 0) { printf("%d unsupported\n", nfft); continue; }
        const FftRouteInfo r = fft_route(nfft, st, ns);
        printf("%d %s %d %d\n", nfft, name(r.route), (int)r.in_place_ok, (int)r.needs_work);
    }
    return 0;
}
