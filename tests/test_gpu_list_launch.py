"""List launches: redio_chain_enqueue_list / redio_fft_enqueue_list run several independent messages in one launch
(chain_v4_list_kernel, fft1k_wave_list_kernel) and must give the bits of one single call per message -- the reference's
per-message pattern, src/kissfft/src/kissfft.rs:20-27 (one block_size message per call).  Also the coalescing graph blocks of
include/kpn_dev.hpp (tests/cpp_list `list_gpu`)."""
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(127, 5), (127, 3), (127, 1), (63, 5), (63, 1)]
GUARD = 64  # complex64 words behind every output
NAN = np.uint32(0x7FC0DEAD)


def u32(a):
    return np.ascontiguousarray(a).view(np.uint32)


def pool(k, d):
    """(n_in, misaligned) of the ragged messages: one block, 12 blocks, 2^20 samples, no block, trailing samples, an 8-byte offset input."""
    one = 1023 * d + k
    return [(one, False), (12 * 1024 * d - d + k, False), (1 << 20, False), (k - 1, False), (one + 3 * d + 700, False), (3 * 1024 * d + k, True)]


def guarded(gpu, nelem):
    buf = gpu.empty(nelem + GUARD, dtype=gpu.complex64, device="cuda")
    buf.view(gpu.int32).fill_(int(NAN.view(np.int32)))
    return buf


@pytest.mark.parametrize("k,d", SHAPES)
@pytest.mark.parametrize("fused", [True, False])
def test_chain_list_bits(gpu, redio, oracle, k, d, fused):
    taps = oracle.lpf_corrected(k, 0.08)
    chain = redio.Chain(taps, d, 1024, fused=fused)
    assert chain.is_fused
    msgs = []
    for j, (n, mis) in enumerate(pool(k, d)):
        x = oracle.synth_iq(0x600D + 31 * j + k + d, 0, n)
        if mis:
            base = gpu.empty(n + 1, dtype=gpu.complex64, device="cuda")
            dx = base[1:]
            dx.copy_(gpu.from_numpy(x))
            assert dx.data_ptr() % 16 == 8
        else:
            dx = gpu.from_numpy(x).cuda()
            assert dx.data_ptr() % 16 == 0
        want = oracle.chain_fir_fft(x, taps, d, 1024, fused=fused)
        msgs.append((dx, want))
    single = [chain(dx) for dx, _ in msgs]
    gpu.cuda.synchronize()
    for (dx, want), s in zip(msgs, single):
        assert np.array_equal(u32(s.cpu().numpy()), u32(want))
    for count in (1, 2, 7, 32, 33):
        entries = [msgs[(i * 5 + count) % len(msgs)] for i in range(count)]
        bufs = [guarded(gpu, w.size) for _, w in entries]
        outs = [b[: w.size].view(w.shape[0], 1024) if w.size else b[:0] for b, (_, w) in zip(bufs, entries)]
        chain.enqueue_list([dx for dx, _ in entries], outs)
        gpu.cuda.synchronize()
        for b, (_, w) in zip(bufs, entries):
            h = b.cpu().numpy()
            assert np.array_equal(u32(h[: w.size]), u32(w).ravel()), f"count {count}: an output differs from the oracle"
            assert np.all(u32(h[w.size:]) == NAN), f"count {count}: a write behind an output"


def test_chain_list_unfused_plan_loops(gpu, redio, oracle):
    taps = oracle.lpf_corrected(127, 0.08)
    chain = redio.Chain(taps, 5, 1024, fused=True)
    chain.set_unfused(True)
    xs = [oracle.synth_iq(7 + i, 0, 5120 * (i + 1) + 126) for i in range(3)]
    outs = chain.enqueue_list([gpu.from_numpy(x).cuda() for x in xs])
    gpu.cuda.synchronize()
    for x, o in zip(xs, outs):
        assert np.array_equal(u32(o.cpu().numpy()), u32(oracle.chain_fir_fft(x, taps, 5, 1024, fused=True)))


def test_chain_list_rejects_in_place(gpu, redio, oracle):
    chain = redio.Chain(oracle.lpf_corrected(127, 0.08), 5, 1024)
    x = gpu.from_numpy(oracle.synth_iq(3, 0, 5246)).cuda()
    with pytest.raises(redio.RedioError):
        chain.enqueue_list([x], [x])


@pytest.mark.parametrize("inverse", [False, True])
@pytest.mark.parametrize("count", [1, 5, 32, 40])
def test_fft1k_list_bits(gpu, redio, oracle, inverse, count):
    fft = redio.Fft(1024, inverse=inverse)
    rng = np.random.default_rng(count + 100 * inverse)
    xs = [oracle.synth_iq(0xF00 + i, 0, 1024 * int(rng.integers(1, 10))) for i in range(count)]
    bufs = [guarded(gpu, x.size) for x in xs]
    fft.enqueue_list([gpu.from_numpy(x).cuda() for x in xs], [b[: x.size] for b, x in zip(bufs, xs)])
    gpu.cuda.synchronize()
    for b, x in zip(bufs, xs):
        h = b.cpu().numpy()
        assert np.array_equal(u32(h[: x.size]), u32(oracle.fft(x, 1024, inverse=inverse)))
        assert np.all(u32(h[x.size:]) == NAN)


@pytest.mark.parametrize("nfft", [256, 1000])
def test_fft_list_other_sizes_loop(gpu, redio, oracle, nfft):
    fft = redio.Fft(nfft)
    xs = [oracle.synth_iq(0xA00 + i, 0, nfft * (i % 4 + 1)) for i in range(6)]
    outs = fft.enqueue_list([gpu.from_numpy(x).cuda() for x in xs])
    gpu.cuda.synchronize()
    for x, o in zip(xs, outs):
        assert np.array_equal(u32(o.cpu().numpy()), u32(oracle.fft(x, nfft)))


def test_chain_list_capture_replays(gpu, redio, oracle):
    taps = oracle.lpf_corrected(127, 0.08)
    chain = redio.Chain(taps, 5, 1024, fused=True)
    xs = [gpu.from_numpy(oracle.synth_iq(50 + i, 0, 5120 * (i % 3 + 1) + 126)).cuda() for i in range(12)]
    want = [o.cpu().numpy() for o in chain.enqueue_list(xs)]
    outs = [gpu.empty_like(gpu.from_numpy(w)).cuda() for w in want]
    gpu.cuda.synchronize()
    m0 = redio.lib().redio_malloc_count()
    g = redio.Graph()
    with g:
        chain.enqueue_list(xs, outs)
    for _ in range(2):
        for o in outs:
            o.zero_()
        g.launch()
        gpu.cuda.synchronize()
        for o, w in zip(outs, want):
            assert np.array_equal(u32(o.cpu().numpy()), u32(w))
    assert redio.lib().redio_malloc_count() == m0


def test_headline_kernel_name_unchanged(gpu, redio, oracle):
    chain = redio.Chain(oracle.lpf_corrected(127, 0.08), 5, 1024, fused=True)
    assert chain.kernel_name == "chain_v4_kernel<127,5,true,2,8,false,true,false,false>"


def test_coalescing_graph_checksums(gpu, redio):
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "tests", "cpp_list"), "-s"])
    out = subprocess.run([os.path.join(ROOT, "tests", "_build", "kpn_list_tests"), "list_gpu"], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr
    lines = [l.split() for l in out.stdout.splitlines() if l.startswith("list_gpu")]
    assert [l[1] for l in lines] == ["chain", "fft"]
    for l in lines:
        assert l[2] == "off" and l[5] == "on"
        assert l[3] == l[6] and l[4] == l[7] and int(l[4]) > 0, l
