"""The polyphase spectrometer under stream capture: a fused plan replays in a Graph with equal bits, an un-reserved generic plan
refuses to allocate inside a capture, and after reserve nothing is allocated.  Then dev::polyphase_spectrum, dev::polyphase_spectrum_u8
and their _stream forms (include/kpn_dev.hpp) in a device-resident graph, through tests/cpp_pfb_pspec: source -> block -> sink
through rings of 1 and 2 buffers on a fused shape (64 x 16, K = 17) and a generic one (128 x 8, K = 5); the sink's rows bit for bit
against the restatement, and no device allocation after the first message."""
import os
import subprocess

import numpy as np
import pytest

import pfb_pspec_ref as ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 0x5EED0F5E
ERR_NOT_RESERVED = -6


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.mark.parametrize("u8", [False, True])
@pytest.mark.parametrize("M,P,K,mode", [(64, 16, 17, 1), (64, 16, 17, 2), (64, 8, 5, 0), (128, 8, 17, 0), (100, 5, 5, 0)])
def test_reserve_then_capture_and_replay(gpu, redio, oracle, M, P, K, mode, u8):
    h = oracle.synth_f32(9, 0, M * P)
    n = M * (5 * K + P - 1) + 3
    plan = redio.PolyphaseSpectrum(h, M, P, K)
    plan.set_split(mode)
    if u8:
        raw = np.random.default_rng(SEED).integers(0, 256, 2 * n, dtype=np.uint8)
        d, want = gpu.from_numpy(raw).cuda(), ref.spectrum_u8(raw, h, M, P, K, True)
    else:
        x = oracle.synth_iq(SEED, 0, n)
        d, want = gpu.from_numpy(x).cuda(), ref.spectrum(x, h, M, P, K, True)
    out = gpu.zeros(want.size, dtype=gpu.float32, device="cuda")
    plan.reserve(n, u8=u8)
    count = redio.lib().redio_malloc_count()
    g = redio.Graph()
    with g:
        (plan.from_bytes if u8 else plan)(d, out=out)
    for _ in range(2):
        out.zero_()
        g.launch()
        gpu.cuda.synchronize()
        assert np.array_equal(bits(out.cpu().numpy()), bits(want.reshape(-1)))
    assert redio.lib().redio_malloc_count() == count  # reserved: the enqueue allocated nothing


def test_fused_row_mode_captures_without_a_reserve(gpu, redio, oracle):
    """a wave per run of whole rows needs no scratch at all"""
    M, P, K = 64, 16, 40
    h = oracle.synth_f32(9, 0, M * P)
    x = oracle.synth_iq(SEED, 1, M * (3 * K + P - 1))
    want = ref.spectrum(x, h, M, P, K, True)
    d = gpu.from_numpy(x).cuda()
    out = gpu.zeros(want.size, dtype=gpu.float32, device="cuda")
    plan = redio.PolyphaseSpectrum(h, M, P, K)
    plan.set_split(plan.ROWS)
    count = redio.lib().redio_malloc_count()
    g = redio.Graph()
    with g:
        plan(d, out=out)
    g.launch()
    gpu.cuda.synchronize()
    assert np.array_equal(bits(out.cpu().numpy()), bits(want.reshape(-1)))
    assert redio.lib().redio_malloc_count() == count


@pytest.mark.parametrize("M,P,K,mode", [(128, 8, 5, 0), (64, 16, 17, 2)])
def test_capture_needs_the_reserve(gpu, redio, oracle, M, P, K, mode):
    """an un-reserved generic plan (its row scratch), and a fused one that leaves segment partials: REDIO_ERR_NOT_RESERVED inside a
    capture, and the plan and the stream work on afterwards"""
    h = oracle.synth_f32(9, 0, M * P)
    x = oracle.synth_iq(SEED, 2, M * (2 * K + P - 1))
    want = ref.spectrum(x, h, M, P, K, True)
    d = gpu.from_numpy(x).cuda()
    out = gpu.zeros(want.size, dtype=gpu.float32, device="cuda")
    plan = redio.PolyphaseSpectrum(h, M, P, K)
    plan.set_split(mode)
    g = redio.Graph()
    with pytest.raises(redio.RedioError) as e:
        with g:
            plan(d, out=out)
    assert e.value.code == ERR_NOT_RESERVED
    assert np.array_equal(bits(plan(d, out=out).cpu().numpy()), bits(want))


SHAPES = [(64, 16, 17), (128, 8, 5)]


def stream_lens(W, H):
    return [W + 2 * H] + [2 * H + 100 if i % 2 else 2 * H - 100 for i in range(10)]


def block_lens(W, H):
    return [W + (rows - 1) * H for rows in (3, 1, 2)] * 4


def driver(*args):
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "tests", "cpp_pfb_pspec"), "-s"])
    out = subprocess.run([os.path.join(ROOT, "tests", "_build", "kpn_pfb_pspec_tests"), *args], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    return out.stdout


@pytest.fixture(scope="module")
def cases(oracle, tmp_path_factory):
    """per shape and input kind: the prototype's and the input file's paths, the stream's rows and the per-message rows, computed once"""
    made = {}
    for M, P, K in SHAPES:
        W, H = ref.shape(M, P, K)
        d = tmp_path_factory.mktemp("pfb_pspec")
        h = oracle.synth_f32(9, 0, M * P)
        proto = str(d / "proto.f32")
        h.tofile(proto)
        sl, bl = stream_lens(W, H), block_lens(W, H)
        n = max(sum(sl), sum(bl))
        raw = np.random.default_rng(SEED + M).integers(0, 256, 2 * n, dtype=np.uint8)
        for kind, x in (("cf32", oracle.synth_iq(SEED, M, n)), ("u8", oracle.data_to_samples(raw))):
            path = str(d / f"input.{kind}")
            (raw if kind == "u8" else x).tofile(path)
            stream = ref.spectrum(x[: sum(sl)], h, M, P, K, True)
            starts = np.cumsum([0] + bl[:-1])
            blocks = np.concatenate([ref.spectrum(x[s: s + m], h, M, P, K, True) for s, m in zip(starts, bl)])
            made[(M, P, K, kind)] = (proto, path, stream, blocks)
    return made


@pytest.mark.parametrize("depth", [1, 2])
@pytest.mark.parametrize("kind", ["cf32", "u8"])
@pytest.mark.parametrize("M,P,K", SHAPES)
def test_stream_blocks(gpu, redio, cases, tmp_path, M, P, K, kind, depth):
    proto, path, want, _ = cases[(M, P, K, kind)]
    out = tmp_path / f"stream{depth}.bin"
    line = driver("stream", str(depth), kind, str(M), str(P), str(K), proto, path, str(out)).split()
    assert want.shape[0] == 3 + 5 * (1 + 3)  # every message completes at least one row
    assert line == ["stream", str(depth), "msgs", "11", "words", str(want.size), "mallocs_after_first", "0"]
    got = np.fromfile(out, np.float32)
    assert np.array_equal(got.view(np.uint32), want.reshape(-1).view(np.uint32))


@pytest.mark.parametrize("depth", [1, 2])
@pytest.mark.parametrize("kind", ["cf32", "u8"])
@pytest.mark.parametrize("M,P,K", SHAPES)
def test_whole_row_message_blocks(gpu, redio, cases, tmp_path, M, P, K, kind, depth):
    proto, path, _, want = cases[(M, P, K, kind)]
    out = tmp_path / f"blocks{depth}.bin"
    line = driver("blocks", str(depth), kind, str(M), str(P), str(K), proto, path, str(out)).split()
    assert want.shape[0] == 4 * (3 + 1 + 2)
    assert line == ["blocks", str(depth), "msgs", "12", "words", str(want.size), "mallocs_after_first", "0"]
    got = np.fromfile(out, np.float32)
    assert np.array_equal(got.view(np.uint32), want.reshape(-1).view(np.uint32))
