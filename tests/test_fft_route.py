"""The complex transform's route (libredio_amd/csrc/fft_route.h) without a GPU: tests/emu_route prints fft_route() for a list of sizes,
and the table below says what it has to print.  The table was written out by reading the dispatch cascade this header replaced
(launch_fft before the kernel file was split), in its order: own-kernel sizes, the compile-time list, the LDS kernels, the multi-pass
powers of two, the tile passes, the global-memory stages.  It is not generated from the code under test."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# nfft: (route, in_place_ok, needs_work)
TABLE = {
    1024: ("wave1k", 1, 0),
    2: ("p2", 1, 0), 4: ("p2", 1, 0), 8: ("p2", 1, 0), 16: ("p2", 1, 0), 32: ("p2", 1, 0), 128: ("p2", 1, 0), 512: ("p2", 1, 0),
    64: ("64", 1, 0),
    256: ("256", 1, 0),
    2048: ("one_wave", 1, 0), 4096: ("one_wave", 1, 0),
    8192: ("four_wave", 1, 0), 16384: ("four_wave", 1, 0),
    6: ("ct", 1, 0), 1000: ("ct", 1, 0), 2025: ("ct", 1, 0), 2160: ("ct", 1, 0), 16200: ("ct", 1, 0),  # first, both sides of the two units' cut, last
    3: ("lds_batched", 1, 0), 5: ("lds_batched", 1, 0),      # radices up to 5, at most 8192 points, not in the list
    7: ("lds", 1, 0), 17: ("lds", 1, 0),                      # a radix above 5: two LDS images
    8190: ("lds", 1, 0),                                      # 2 3^2 5 7 13: 2 * 8190 * 8 = 131040 bytes <= 128 KiB
    8191: ("lds", 1, 0),                                      # prime: 131056 bytes
    8194: ("global", 0, 1),                                   # 2 17 241: 131104 bytes, one step beyond LDS
    16385: ("global", 0, 1),                                  # 5 29 113
    32768: ("multipass", 0, 0), 65536: ("multipass", 0, 0), 1 << 24: ("multipass", 0, 0),
    1 << 25: ("global", 0, 0), 1 << 26: ("global", 0, 0),     # beyond the multi-pass tables, and no tile passes for a power of two
    49152: ("tile_passes", 0, 0),                             # 3 2^14
    16875: ("tile_passes", 0, 0),                             # 3^3 5^4: the first radix-3/5 size above 16384
}


def test_route_table():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "tests", "emu_route"), "-s"])
    sizes = sorted(TABLE)
    out = subprocess.run([os.path.join(ROOT, "tests", "_build", "route_table"), *map(str, sizes)], capture_output=True, text=True, check=True).stdout
    got = {}
    for line in out.splitlines():
        n, route, in_place_ok, needs_work = line.split()
        got[int(n)] = (route, int(in_place_ok), int(needs_work))
    assert got == TABLE
