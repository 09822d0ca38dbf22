"""A/B of the headline chain kernel (block schedule 1 of chain_v4_body) against schedule 2 (chain_v4_sched2_kernel: the transform of
block b under the first FIR of block b + 1, exchanges in halves behind the image), interleaved in ONE process on one box: the
measurement build (make -C libredio_amd/csrc measure) selects the form per launch from REDIO_CHAIN_SCHED2.  Bit comparison on 2^28
samples and on sizes whose runs are 1, 2, 3 and 4 blocks with a shorter last run.  usage: python3 tools/chain_sched_ab.py [rounds]"""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault("REDIO_BUILD_DIR", os.path.join(ROOT, "libredio_amd", "_build_measure"))
import torch, libredio_amd as R

rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 3
taps = R.dsputils.lpf_corrected(127, 0.08)
plan = R.Chain(taps, 5, 1024, fused=True)
plan_ref = R.Chain(taps, 5, 1024, fused=False)


def run(p, x, out, sched2):
    if sched2: os.environ["REDIO_CHAIN_SCHED2"] = "1"
    else: os.environ.pop("REDIO_CHAIN_SCHED2", None)
    p(x, out=out)


# bits first: both roundings
for nb in (1, 5, 13, 24579, 36866, 49155):
    n = nb * 5120 + 126 + 17
    x = R.synth_iq(0x5EED0002, 7, n)
    for p in (plan, plan_ref):
        assert p.nblocks(n) == nb
        a = torch.zeros((nb, 1024), dtype=torch.complex64, device="cuda"); b = torch.zeros_like(a)
        run(p, x, a, False); run(p, x, b, True)
        torch.cuda.synchronize()
        same = torch.equal(a.view(torch.int32), b.view(torch.int32))
        print(f"{nb} blocks, runs of {p.blocks_per_wave(nb)}, {'fmaf' if p is plan else 'reference rounding'}: schedule 2 has the same bits: {same}", flush=True)
        assert same
    del x

n = 1 << 28
x = R.synth_iq(0x5EED0002, 0, n)
out = torch.empty((plan.nblocks(n), 1024), dtype=torch.complex64, device="cuda")
alg = 9.6 * plan.nblocks(n) * 5120
for p, what in ((plan, "fmaf"), (plan_ref, "reference rounding")):
    for r in range(rounds):
        for s2 in (False, True):
            for _ in range(300): run(p, x, out, s2)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(300): run(p, x, out, s2)
            e1.record(); torch.cuda.synchronize()
            ms = e0.elapsed_time(e1) / 300
            print(f"{what}, round {r}: {'schedule 2 (transform under the next FIR)' if s2 else 'schedule 1 (product form)               '}: {ms:.4f} ms = {alg / ms / 1e6 / 80:.2f} % of 8 TB/s", flush=True)
