"""The watermark rule on the host alone (tests/watermark_ref.py; include/mimi_hip.h states it): the streamed restatement equals the
whole-clip embed over every length and schedule, what each part of the rule decides, recovery after damage, the SDR on a synthetic voice,
and known answers stored under tests/golden/ so that the rule cannot drift."""
import json
import os

import numpy as np
import pytest

import watermark_ref as W

S, K, P = W.S, W.K, W.P
LENGTHS = [0, 1, 1919, 1920, 1921, 3839, 5767, P - 1, P, P + S + 5]
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "watermark_known.json")
_cache = {}


def clip(n, seed=0, int16=False):
    """n samples of a voiced signal over hiss (cheap: two harmonics under an envelope)"""
    g = np.random.default_rng(seed * 7919 + n)
    t = np.arange(n) / 24000.0
    x = (0.25 * np.sin(2 * np.pi * 140.0 * t + seed) + 0.1 * np.sin(2 * np.pi * 433.0 * t)) * (0.6 + 0.4 * np.sin(2 * np.pi * 3.0 * t))
    x = (x + 0.003 * g.standard_normal(n)).astype(np.float32)
    return np.clip(np.rint(x * 32768), -32768, 32767).astype(np.int16) if int16 else x


def schedules(n, seed=0):
    """Three ways to cut n samples: random draws; everything, then final alone; single samples around a block edge.
    -> [(chunk lengths fed without final, whether what is left goes with final or final comes alone)]"""
    g = np.random.default_rng(seed + n)
    draws, left = [], n
    while left > 0:
        d = min(int(g.choice([0, 1, 7, 1919, 1920, 4000])), left)
        draws.append(d)
        left -= d
    whole = [n]
    edge = ([min(n, S - 2)] + [1] * min(max(n - (S - 2), 0), 4)) if n else []
    edge = edge + ([n - sum(edge)] if n - sum(edge) > 0 else [])
    return [draws, whole, edge]


def cut(x, parts):
    out, at = [], 0
    for d in parts:
        out.append(x[at:at + d])
        at += d
    assert at == len(x)
    return out


def bits_equal(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.int32 if a.dtype == np.float32 else a.dtype), b.view(np.int32 if b.dtype == np.float32 else b.dtype))


def voice():
    if "voice" not in _cache:
        x = W.synthetic_voice(10.0)
        _cache["voice"] = (x, W.embed(x))
    return _cache["voice"]


def damaged(y, seed=1):
    """scaled by 0.7, re-quantised to 16 bits, noise at 0.001 added"""
    z = np.clip(np.rint(y * np.float32(0.7) * 32768), -32768, 32767) / 32768.0
    return (z + 0.001 * np.random.default_rng(seed).standard_normal(len(z))).astype(np.float32)


@pytest.mark.parametrize("int16", [False, True])
@pytest.mark.parametrize("n", LENGTHS)
def test_streaming_equals_whole_clip(n, int16):
    x = clip(n, 1, int16)
    want = W.embed(x, t_q4=8)
    assert bits_equal(want[n // S * S:], x[n // S * S:]), "the trailing partial block is left as it is"
    for parts in schedules(n):
        st = W.StreamEmbed(t_q4=8)
        got = [st.feed(c) for c in cut(x, parts)]
        lag = sum(parts) - sum(len(g) for g in got)
        assert 0 <= lag < S, "the output lags the input by less than one block"
        got.append(st.feed(x[:0], final=True))
        assert len(got[-1]) == n % S and bits_equal(got[-1], x[n - n % S:]), "the final tail comes through unchanged"
        assert bits_equal(np.concatenate(got), want), (n, parts[:6])
        assert st.pos == 0 and st.carry is None


def test_ten_frame_chunks_lag_by_nothing():
    x = clip(3 * 19200, 2)
    st = W.StreamEmbed()
    for c in cut(x, [19200] * 3):
        assert len(st.feed(c)) == 19200


def test_the_remainder_spread_makes_the_push_exact():
    x, c, b = W.quant(clip(S, 3)), W.chips()[:S], int(W.symbols()[0])
    d, D = W.block_push(x, c, b, 8)
    assert D != 0 and abs(D) % S != 0 and int((d * c).sum()) == D
    flat, _ = W.block_push(x, c, b, 8, spread=False)
    assert int((flat * c).sum()) != D


def test_t_q4_zero_loses_symbols_to_the_tie_at_zero():
    x, y = voice()
    assert W.detect(y, W.DEFAULT_PAYLOAD, n_off=1)[2] == K
    row = W.detect(W.embed(x, t_q4=0), W.DEFAULT_PAYLOAD, n_off=1)
    assert row[2] < K and row[3] == K


def test_the_wrong_secret_scores_no_better_than_an_unmarked_clip():
    x, y = voice()
    plain = W.detect(x, W.DEFAULT_PAYLOAD, n_off=1)
    wrong = W.detect(y, W.DEFAULT_PAYLOAD, secret=12345, n_off=1)
    # chance: 56 fair coins, sd 3.74 -- both lie within four of them of 28 and neither verifies
    assert abs(int(wrong[2]) - 28) <= 15 and abs(int(plain[2]) - 28) <= 15
    assert not W.verify_row(wrong) and not W.verify_row(plain)


def test_a_cut_clip_is_found_at_its_offset_and_nowhere_beside_it():
    _, y = voice()
    c = y[1000:1000 + 5 * 24000]
    row = W.detect(c, W.DEFAULT_PAYLOAD, o0=990, n_off=21)
    assert row[0] == 10 and row[1] == 1000 and row[2] == K and row[3] == K and row[6] == 1
    assert row[5] == W.default_secret() and row[4] == (len(c) - (-1000) % S) // S
    for o in (999, 1001):
        beside = W.detect(c, W.DEFAULT_PAYLOAD, o0=o, n_off=1)
        assert abs(int(beside[2]) - 28) <= 15 and not W.verify_row(beside)


def test_silence_in_gives_silence_out():
    for z in (np.zeros(5 * S + 3, np.float32), np.zeros(5 * S + 3, np.int16)):
        assert bits_equal(W.embed(z), z)
    row = W.detect(np.zeros(4 * S, np.float32), W.DEFAULT_PAYLOAD, o0=5, n_off=9)
    assert row[0] == 0 and row[1] == 5 and row[2] == 0 and row[6] == 0 and not row[8:].any(), "every offset scores 0: the first one is the best"


def test_non_finite_samples_stay_and_count_as_zero():
    x = clip(2 * S, 4)
    bad = x.copy()
    bad[[5, 700, S + 9]] = [np.nan, np.inf, -np.inf]
    hole = x.copy()
    hole[[5, 700, S + 9]] = 0.0
    y, yh = W.embed(bad), W.embed(hole)
    assert np.isnan(y[5]) and y[700] == np.inf and y[S + 9] == -np.inf
    assert bits_equal(y[[5, 700, S + 9]], bad[[5, 700, S + 9]]), "what it was, bit for bit"
    keep = np.ones(2 * S, bool)
    keep[[5, 700, S + 9]] = False
    # (a zero sample may itself be pushed, a non-finite one is not: everywhere else the two clips get the same push)
    assert bits_equal(y[keep], yh[keep])
    assert np.array_equal(W.quant(bad), W.quant(hole))


def test_recovery_after_damage_and_no_false_alarm():
    x, y = voice()
    row = W.detect(damaged(y), W.DEFAULT_PAYLOAD, n_off=1)
    assert row[2] == K and row[3] == K and row[6] == 1 and W.verify_row(row)
    assert not W.verify_row(W.detect(x, W.DEFAULT_PAYLOAD, n_off=1))
    assert not W.verify_row(W.detect(damaged(x), W.DEFAULT_PAYLOAD, o0=0, n_off=64))


def test_sdr_on_the_synthetic_voice():
    x, y = voice()
    x64, y64 = x.astype(np.float64), y.astype(np.float64)
    sdr = 10 * np.log10((x64 ** 2).sum() / ((y64 - x64) ** 2).sum())
    print(f"SDR at t_q4 = 8: {sdr:.2f} dB")
    assert sdr >= 31.0


def test_verify_rule():
    row = np.zeros(64, np.int64)
    for score, covered, want in ((56, 56, True), (49, 56, True), (48, 56, False), (16, 16, True), (14, 16, True), (13, 16, False), (15, 15, False), (0, 0, False)):
        row[2], row[3] = score, covered
        assert W.verify_row(row) is want, (score, covered)


def test_known_answers():
    known = json.load(open(GOLDEN))
    assert W.crc8(known["payload"]) == known["crc8"] and list(W.DEFAULT_PAYLOAD) == known["payload"]
    assert W.chips()[:64].tolist() == known["chips"]
    assert W.symbol_bits() == known["symbol_bits"] and W.default_secret() == known["secret"]
    assert W.crc8(b"123456789") == 0xF4, "CRC-8 (poly 0x07, init 0): the catalogue's check value"
