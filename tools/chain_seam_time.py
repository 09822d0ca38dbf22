"""Kernel time of the headline chain (127 taps / 5 -> 1024 points, 2^28 samples), its reference-rounding twin and its u8 entry in the
build REDIO_BUILD_DIR selects: 3 x (300 warm-up + 300 timed launches) each, HIP events, and the sum of the output's 32-bit words so
that two builds can be seen to write the same bits.  usage: python3 tools/chain_seam_time.py [tag]   (tools/chain_seam_ab.sh)"""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch, libredio_amd as R

tag = sys.argv[1] if len(sys.argv) > 1 else os.path.basename(os.environ.get("REDIO_BUILD_DIR", "product"))
n = 1 << 28
taps = R.dsputils.lpf_corrected(127, 0.08)
x = R.synth_iq(0x5EED0002, 0, n)
raw = torch.randint(0, 256, (2 * n,), dtype=torch.uint8, device="cuda", generator=torch.Generator(device="cuda").manual_seed(0x5EA))
for what, fused, u8 in (("fmaf", True, False), ("reference rounding", False, False), ("u8 fmaf", True, True)):
    plan = R.Chain(taps, 5, 1024, fused=fused)
    out = torch.empty((plan.nblocks(n), 1024), dtype=torch.complex64, device="cuda")
    run = (lambda: plan.from_bytes(raw, out=out)) if u8 else (lambda: plan(x, out=out))
    ms = []
    for _ in range(3):
        for _ in range(300): run()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(300): run()
        e1.record(); torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1) / 300)
    checksum = int(out.view(torch.int32).to(torch.int64).sum().item())
    print(f"{tag}: {what:18s} ms " + " ".join(f"{m:.4f}" for m in ms) + f"  checksum {checksum}", flush=True)
    del out
