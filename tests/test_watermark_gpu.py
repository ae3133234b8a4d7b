"""The device watermark pool (include/mimi_hip.h mimi_wm_pool_*, sesameai/watermarking.py) against the rule (tests/watermark_ref.py): every
comparison is bit for bit -- embed one-shot and streamed over the oracle test's schedules, fp32 and int16, in any company and order, across
the period's wrap and with forced remainders; detect's whole 64-value row over windows of every size around the tile, across the wrap, on
odd and even offsets, short, silent and many clips and the full period; and one ``generate_many_stream(watermark=)`` run end to end."""
import numpy as np
import pytest
import torch

import watermark_ref as W
from test_watermark_oracle import LENGTHS, bits_equal, clip, cut, schedules

pytestmark = pytest.mark.gpu
S, K, P = W.S, W.K, W.P
_cache = {}


def _pool(n=64, secret=None):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from sesameai.watermarking import WatermarkPool
    if (n, secret) not in _cache:
        _cache[(n, secret)] = WatermarkPool(n, secret)
    return _cache[(n, secret)]


def _t(x):
    return torch.from_numpy(np.ascontiguousarray(x))


def _same(got, want, what):
    got = got.cpu().numpy()
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, got.shape, want.shape)
    assert bits_equal(got, want), (what, int(np.count_nonzero(got != want)), np.flatnonzero(got != want)[:5].tolist())


def _marked(n_blocks=8, seed=5, int16=False):
    """a marked stream of n_blocks blocks (the reference's), cached"""
    if ("marked", n_blocks, seed, int16) not in _cache:
        _cache[("marked", n_blocks, seed, int16)] = W.embed(clip(n_blocks * S, seed, int16))
    return _cache[("marked", n_blocks, seed, int16)]


@pytest.mark.parametrize("int16", [False, True])
def test_embed_one_stream_every_length(int16):
    pool = _pool()
    for n in LENGTHS:
        x = clip(n, 1, int16)
        (got,) = pool.embed([_t(x)])
        _same(got, W.embed(x), n)


def test_embed_64_streams_of_different_lengths_payloads_and_thresholds_in_one_launch():
    pool = _pool()
    g = np.random.default_rng(11)
    lens = [0, 1, S - 1, S, S + 1] + [int(v) for v in g.integers(2, 6 * S, 59)]
    pays = [[int(b) for b in g.integers(0, 256, 5)] for _ in lens]
    ts = [1 + i for i in range(64)]
    clips = [clip(n, i) for i, n in enumerate(lens)]
    got = pool.embed([_t(c) for c in clips], pays, ts)
    for i, (c, y) in enumerate(zip(clips, got)):
        _same(y, W.embed(c, pays[i], secret=pool.secret, t_q4=ts[i]), i)


def test_a_stream_alone_in_company_and_in_another_order_gives_the_same_bits():
    pool = _pool()
    clips = [clip(3 * S + 17 * i, i) for i in range(6)]
    want = [W.embed(c) for c in clips]
    ids = [9, 3, 40, 63, 0, 21]
    pool.reset(ids)
    for y, w in zip(pool.feed(ids, [_t(c) for c in clips], True), want):
        _same(y, w, "company")
    order = [4, 2, 5, 0, 3, 1]
    pool.reset([ids[j] for j in order])
    for j, y in zip(order, pool.feed([ids[j] for j in order], [_t(clips[j]) for j in order], True)):
        _same(y, want[j], "another order")
    pool.reset([17])
    _same(pool.feed([17], [_t(clips[2])], True)[0], want[2], "alone, on another stream id")


@pytest.mark.parametrize("int16", [False, True])
def test_embed_streamed_over_three_schedules(int16):
    """Streams of different lengths share the calls, each on its own schedule; one crosses the period's wrap at P."""
    pool = _pool()
    lens = [1, 1919, 1920, 1921, 5767, P + S + 5]
    for which in range(3):
        clips = [clip(n, 3, int16) for n in lens]
        parts = [cut(c, schedules(len(c), seed=which)[which]) for c in clips]
        ids = [5 * i + which for i in range(len(lens))]
        pool.reset(ids)
        got = [[] for _ in ids]
        for t in range(max(len(p) for p in parts) + 1):
            live = [j for j in range(len(ids)) if t <= len(parts[j])]
            fin = [t == len(parts[j]) for j in live]
            chunks = [_t(parts[j][t]) if t < len(parts[j]) else _t(clips[j][:0]) for j in live]
            counts = [pool.out_count(ids[j], len(c), f) for j, c, f in zip(live, chunks, fin)]
            ys = pool.feed([ids[j] for j in live], [c.cuda() for c in chunks], fin)
            assert [int(y.shape[0]) for y in ys] == counts
            for j, y in zip(live, ys):
                got[j].append(y)
        for j, c in enumerate(clips):
            fed = sum(len(p) for p in parts[j])
            assert fed == len(c) and sum(int(y.shape[0]) for y in got[j][:-1]) > fed - S, "the output lags by less than one block"
            _same(torch.cat(got[j]), W.embed(c), (which, lens[j]))


def test_forced_remainders_of_zero_and_of_s_minus_one():
    """q = -b A c makes r = -b A S, so |D| = T + A S and rem = T % S with T = (isqrt(A^2 S) * t_q4) >> 4: scan A and t_q4 for both ends."""
    import math
    pool = _pool()
    c0, b0 = W.chips()[:S], int(W.symbols()[0])
    for rem in (0, S - 1):
        A, t = next((A, t) for A in range(1, 3000) for t in range(1, 65) if ((math.isqrt(A * A * S) * t) >> 4) % S == rem and (math.isqrt(A * A * S) * t) >> 4 > 0)
        x = (-b0 * A * c0).astype(np.int16)
        d, D = W.block_push(x.astype(np.int64), c0, b0, t)
        assert abs(D) % S == rem and D != 0
        for arr in (x, (x / 32768.0).astype(np.float32)):
            (got,) = pool.embed([_t(arr)], W.DEFAULT_PAYLOAD, t)
            _same(got, W.embed(arr, t_q4=t), (rem, arr.dtype))


def _row(pool, x, payload, o0, n_off):
    return pool.detect([_t(x)], payload, search=(o0, n_off), want_rows=True)[0].cpu().numpy()


@pytest.mark.parametrize("true_offset", [1000, 2777])
def test_detect_windows_of_every_size_around_a_tile(true_offset):
    pool = _pool()
    y = _marked()[true_offset:true_offset + 5 * S]                          # four complete blocks at the true offset
    for n_off, o0 in ((1, true_offset), (255, true_offset - 200), (256, true_offset - 255), (257, true_offset - 256), (4096, true_offset - 3000 + P)):
        got, want = _row(pool, y, W.DEFAULT_PAYLOAD, o0, n_off), W.detect(y, W.DEFAULT_PAYLOAD, o0=o0, n_off=n_off)
        assert np.array_equal(got, want), (n_off, got[:8], want[:8])
        if n_off == 1:                                                      # (a wide window over so few symbols may hold an earlier tie)
            assert want[1] == true_offset and want[2] == want[3] == 4 and want[5] == 0


def test_detect_a_window_across_the_wrap_and_int16():
    pool = _pool()
    long = W.embed(clip(P + 6 * S, 6, True))
    for at in (P - 31, P + 50):                                            # the true offset lies on either side of the wrap
        y = long[at:at + 3 * S + 11]
        got, want = _row(pool, y, W.DEFAULT_PAYLOAD, P - 100, 300), W.detect(y, W.DEFAULT_PAYLOAD, o0=P - 100, n_off=300)
        assert np.array_equal(got, want), (at, got[:8], want[:8])
        here = W.detect(y, W.DEFAULT_PAYLOAD, o0=at % P, n_off=1)
        assert here[2] == here[3] >= 2 and want[2] >= here[2], "every complete block at the true offset says its bit"


def test_detect_short_single_block_and_silent_clips():
    pool = _pool()
    y = _marked()
    cases = [(y[:S - 1], 0, 300), (y[:S], 0, 300), (y[S:2 * S], S - 3, 7), (np.zeros(3 * S, np.float32), 5, 600), (y[:0], 0, 3)]
    for x, o0, n_off in cases:
        got, want = _row(pool, x, W.DEFAULT_PAYLOAD, o0, n_off), W.detect(x, W.DEFAULT_PAYLOAD, o0=o0, n_off=n_off)
        assert np.array_equal(got, want), (len(x), got[:8], want[:8])
    assert W.detect(y[:S - 1], W.DEFAULT_PAYLOAD, n_off=300)[3] == 0, "a clip shorter than one block covers nothing"
    silent = W.detect(np.zeros(3 * S, np.float32), W.DEFAULT_PAYLOAD, o0=5, n_off=600)
    assert silent[0] == 0 and silent[2] == 0, "equal scores: the smallest i"


def test_detect_64_clips_of_different_lengths_in_one_call_and_any_payload():
    pool = _pool()
    y = _marked(12, 8)
    g = np.random.default_rng(3)
    at = [int(v) for v in g.integers(0, 5 * S, 64)]
    lens = [int(v) for v in g.integers(0, 6 * S, 64)]
    clips = [y[a:a + n] for a, n in zip(at, lens)]
    search = [(max(a - 20 - i, 0), 30 + 5 * i) for i, a in enumerate(at)]
    for payload in (W.DEFAULT_PAYLOAD, None):                              # all 56 symbols; the sync byte alone
        got = pool.detect([_t(c) for c in clips], payload, search=search, want_rows=True).cpu().numpy()
        for i, c in enumerate(clips):
            want = W.detect(c, payload, o0=search[i][0], n_off=search[i][1])
            assert np.array_equal(got[i], want), (i, payload, got[i][:8], want[:8])


def test_detect_the_full_period():
    pool = _pool()
    y = _marked()[2 * S + 333:2 * S + 333 + 3 * S + 7]
    got, want = _row(pool, y, W.DEFAULT_PAYLOAD, 0, P), W.detect(y, W.DEFAULT_PAYLOAD, o0=0, n_off=P)
    assert np.array_equal(got, want), (got[:8], want[:8])
    assert want[2] == 3 and want[0] <= 2 * S + 333


def test_refusals_leave_the_pool_usable():
    from sesameai._abi import CsmError
    pool = _pool()
    x = _t(clip(S + 5, 9))
    with pytest.raises(CsmError, match="t_q4"):
        pool.reset([0], W.DEFAULT_PAYLOAD, 65)
    with pytest.raises(CsmError, match="duplicate"):
        pool.feed([1, 1], [x, x])
    pool.reset([2])
    pool.feed([2], [x])
    with pytest.raises(CsmError, match="format"):
        pool.feed([2], [x.to(torch.int16)])
    with pytest.raises(CsmError, match="n_off"):
        pool.detect([x], W.DEFAULT_PAYLOAD, search=(0, 0))
    _same(torch.cat([pool.embed([x])[0]]), W.embed(x.numpy()), "after the refusals")


def test_generate_many_stream_marks_every_request_and_verify_tells():
    """Each request's chunks, concatenated, are embed of the unmarked run's; verify is true on them and false on the unmarked run.
    The synthetic codec's weights give audio of O(1) with peaks of 10 -- measured on an MI355X: samples of 1.10 and 1.37 in the first chunk,
    a peak of 1.2531 after a scale of 1/8 -- which the rule's q = clamp(..) saturates; a push on a saturated sample is lost to the detector,
    and verify on the unscaled clip was False.  A real codec's output lies in the PCM range, so the test scales the synthetic codec's last
    convolution by 1/16 and asserts that the clip is in range."""
    from sesameai.generator import Generator, Segment
    from sesameai.mimi import MimiCodec, mimi_tiny_args, synthetic_state_dict
    from sesameai.models import Model, csm_tiny_args
    from sesameai.watermarking import CSM_1B_GH_WATERMARK, load_watermarker, verify, watermark
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    lens = [58, 3, 10, 0, 14]
    sd = synthetic_state_dict(mimi_tiny_args(), seed=4321)
    for name in ("seanet.conv_out.weight", "seanet.conv_out.bias"):
        sd[name] = sd[name] * 0.0625
    codec = MimiCodec(mimi_tiny_args(), sd, max_frames=64)
    model = Model(csm_tiny_args(), None, max_frames=64, max_prefill_rows=128)
    gen = Generator(model, audio_tokenizer=codec, max_batch_size=3)
    gen.refill_row_layers = 10
    g = torch.Generator().manual_seed(21)
    texts = [torch.randint(0, 1000, (4 + i % 5,), generator=g).tolist() for i in range(len(lens))]
    ctxs = [[Segment(speaker=1, text=torch.randint(0, 1000, (3,), generator=g).tolist(), audio_codes=torch.randint(0, 2048, (32, 2 + i % 4), generator=g))]
            for i in range(len(lens))]

    def run(**kw):                                          # greedy (top-k 1): every run generates the same frames
        got = {i: [] for i in range(len(lens))}
        for i, pcm, frames, last in gen.generate_many_stream(texts, [1] * len(lens), ctxs, max_audio_length_ms=[n * 80 for n in lens], temperature=0.9,
                                                             topk=1, first_chunk_frames=2, **kw):
            got[i].append(pcm.clone())
        return {i: torch.cat(c) for i, c in got.items()}
    plain, marked = run(), run(watermark=True)
    wm = load_watermarker("cuda", kind="device")
    for i, n in enumerate(lens):
        assert plain[i].shape[0] == marked[i].shape[0] == n * S
        _same(marked[i], W.embed(plain[i].cpu().numpy()), f"request {i}")
    assert not torch.equal(plain[0], marked[0]) and float(plain[0].abs().max()) < 1.0, "the clip lies in the PCM range"
    assert verify(wm, marked[0], 24000, CSM_1B_GH_WATERMARK) and not verify(wm, plain[0], 24000, CSM_1B_GH_WATERMARK)
    assert verify(wm, marked[0][777:], 24000, CSM_1B_GH_WATERMARK), "cut at the front: found at another offset"
    again, rate = watermark(wm, plain[0], 24000, CSM_1B_GH_WATERMARK)
    assert rate == 24000 and torch.equal(again, marked[0]), "the module's watermark() is the same mark"
    assert verify(None, marked[0], 24000, CSM_1B_GH_WATERMARK) is False
