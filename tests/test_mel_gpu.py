"""The device's Whisper log-mel streams (include/mimi_hip.h mimi_mel_pool_*, sesameai/mel.py) against the rule (tests/mel_ref.py, float64)
and against what transformers' WhisperFeatureExtractor gave the same seeded inputs (tests/golden/mel.pt, tools/mel_golden.py; E is the
largest distance of the extractor from the rule over the fixture's inputs).

The bounds.  An fp32 k-ordered fmaf chain lies 0.23 - 0.60 E_i from the rule, so a correct kernel sits inside 1 E of mel_ref; the device
is held to 2 E against mel_ref and to 3 E (2 E plus the extractor's own E) against the stored extractor features.  Each of six plausible
faults moves the features by more than 20 x 2 E (tests/test_mel_oracle.py).  Streaming against one-shot is torch.equal throughout."""
import os

import numpy as np
import pytest
import torch

import mel_ref as R

pytestmark = pytest.mark.gpu
_cache = {}
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mel.pt")


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _fixture():
    if "fix" not in _cache:
        _cache["fix"] = torch.load(GOLDEN)
    return _cache["fix"]


def _input(i):
    """(the clip, the rule's features, the device's features and raw rows) of fixture input i, each computed once"""
    if ("in", i) not in _cache:
        from sesameai.mel import MelPool, log_mel
        it = _fixture()["inputs"][i]
        x = R.signal(it["name"], it["seed"], it["length"])
        assert (x.dtype == np.int16) == (it["fmt"] == "int16")
        _cache[("in", i)] = (x, R.log_mel(x, it["n_mels"]), log_mel([torch.from_numpy(x)], it["n_mels"])[0].cpu())
    return _cache[("in", i)]


def _pool(n=64, n_mels=80):
    from sesameai.mel import MelPool
    if ("pool", n, n_mels) not in _cache:
        _cache[("pool", n, n_mels)] = MelPool(n, n_mels)
    return _cache[("pool", n, n_mels)]


def _clip(n, seed, i16=False):
    x = R.signal("speech", seed, n)
    return torch.from_numpy(np.round(x * 32767.0).astype(np.int16) if i16 else x)


def _one_shot(x, n_mels=80, sid=0):
    """(raw rows, features) of a clip on a fresh stream, in one feed with final"""
    key = ("one", x.data_ptr(), int(x.shape[0]), n_mels)
    if key not in _cache:
        p = _pool(64, n_mels)
        p.reset([sid])
        (raw,) = p.feed([sid], [x], True)
        _cache[key] = (raw.clone(), p.finish([raw])[0].clone(), x)
    return _cache[key][:2]


def _chunks(n, sizes):
    out, at, k = [], 0, 0
    while at < n:
        out.append((at, min(n, at + sizes[k % len(sizes)])))
        at, k = out[-1][1], k + 1
    return out


@pytest.mark.parametrize("n_mels", [80, 128])
def test_tables_read_back_against_the_rule(n_mels):
    _need_gpu()
    w, b, f = _pool(4, n_mels).tables()
    c, ms = R.basis()
    half_ulp = 2.0 ** -24 * (1 + 1e-6)                                   # fp32 rounding of a value of at most 1
    assert np.abs(w.numpy().astype(np.float64) - R.window()).max() <= half_ulp
    assert np.abs(b[:, :201].numpy().astype(np.float64) - c).max() <= half_ulp
    assert np.abs(b[:, 224:425].numpy().astype(np.float64) - ms).max() <= half_ulp
    assert not b[:, 201:224].any() and not b[:, 425:].any()
    want = R.bank(n_mels)
    got = f[:201, :n_mels].numpy().astype(np.float64)
    assert want.max() < 1.0 and np.abs(got - want).max() <= half_ulp * want.max() and (got.sum(axis=0) > 0).all()
    assert not f[201:].any() and not f[:, n_mels:].any()


@pytest.mark.parametrize("i", range(len(R.GOLDEN_INPUTS)))
def test_log_mel_of_every_fixture_input(i):
    """max |device - mel_ref| <= 2 E and max |device - stored extractor| <= 3 E; both figures are printed first."""
    _need_gpu()
    fix = _fixture()
    it, E = fix["inputs"][i], fix["E"]
    assert (it["name"], it["seed"], it["length"], it["n_mels"]) == R.GOLDEN_INPUTS[i]
    x, ref, got = _input(i)
    assert got.shape == (it["n_mels"], 3000) and got.dtype == torch.float32
    d_ref = float(np.abs(got.numpy().astype(np.float64) - ref.astype(np.float64)).max())
    frames = it["frames"].long()
    d_ext = float((got[:, frames].double() - it["features"].double()).abs().max())
    live = it["live"]
    if live < 3000:
        d_ext = max(d_ext, float((got[:, live:].double() - it["constant"]).abs().max()))
        assert (got[:, live:] == got[0, live]).all()
    print(f"input {i} {it['name']} L {it['length']} n_mels {it['n_mels']}: |dev - ref| = {d_ref:.3e} = {d_ref / E:.3f} E "
          f"({d_ref / it['E']:.3f} E_i), |dev - extractor| = {d_ext:.3e} = {d_ext / E:.3f} E")
    assert d_ref <= 2 * E
    assert d_ext <= 3 * E


def test_a_frame_of_zeros_is_exactly_minus_ten():
    _need_gpu()
    raw, feats = _one_shot(torch.zeros(1000), 80, sid=3)
    assert raw.shape == (8, 80) and (raw == -10.0).all() and (feats == -1.5).all()


SCHEDULES = [[1], [159], [160], [161], [4000], [7, 0, 350, 1, 160, 0, 0, 2222, 159, 41]]


@pytest.mark.parametrize("n_mels,i16", [(80, False), (128, True)])
def test_streaming_equals_one_shot(n_mels, i16):
    """Every chunk schedule, alone and among 63 others, in shuffled list order, on another stream id: torch.equal on rows and features."""
    _need_gpu()
    p = _pool(64, n_mels)
    n = 9000
    x = _clip(n, 31, i16)
    raw1, feat1 = _one_shot(x, n_mels)
    assert raw1.shape[0] == R.frames_needed(n, True)
    others = [_clip(3000 + 37 * k, 100 + k, i16) for k in range(63)]
    rng = np.random.RandomState(5)
    for k, sizes in enumerate(SCHEDULES):
        short = sizes == [1]
        xs = x[:700] if short else x                                      # sample by sample over the first frames only: 700 calls
        sid = (7 * k + 3) % 64
        company = k % 2 == 1 and not short
        ids = [sid] + ([s for s in range(64) if s != sid] if company else [])
        p.reset(ids)
        rows, cuts = [], _chunks(len(xs), sizes)
        for c, (a, b) in enumerate(cuts):
            last = c == len(cuts) - 1
            order = list(rng.permutation(len(ids))) if company else [0]
            feed = {ids[0]: xs[a:b]}
            for j, s in enumerate(ids[1:]):
                o = others[j]
                feed[s] = o[min(len(o), 50 * c):min(len(o), 50 * (c + 1))]
            want = p.frame_count(sid, b - a, last)
            out = p.feed([ids[j] for j in order], [feed[ids[j]] for j in order], [last and ids[j] == sid for j in order])
            got = out[order.index(0)]
            assert got.shape == (want, n_mels)
            rows.append(got.clone())
        rows = torch.cat(rows)
        if short:
            raw_s, feat_s = _one_shot(xs, n_mels)
            assert torch.equal(rows, raw_s)
        else:
            assert torch.equal(rows, raw1), sizes
            assert torch.equal(p.finish([rows])[0], feat1)


def test_reuse_after_final_and_reset_empty_chunks_and_an_empty_final():
    _need_gpu()
    p = _pool(64, 80)
    x, y = _clip(5000, 41), _clip(2345, 42)
    rx, _ = _one_shot(x)
    ry, _ = _one_shot(y)
    p.reset([9])
    a = p.feed([9], [x[:1234]], False)[0].clone()
    e = p.feed([9], [x[:0]], False)[0]
    assert e.shape == (0, 80)
    b = p.feed([9], [x[1234:]], False)[0].clone()
    c = p.feed([9], [x[:0]], True)[0].clone()                              # final with no samples: the tail comes out
    assert torch.equal(torch.cat([a, b, c]), rx) and c.shape[0] == rx.shape[0] - R.frames_needed(5000, False)
    assert torch.equal(p.feed([9], [y], True)[0], ry)                      # fresh after final
    p.feed([9], [x[:3000]], False)
    p.reset([9])                                                           # ... and after a reset in mid-clip
    assert torch.equal(p.feed([9], [y], True)[0], ry)
    p.reset([9])
    z = p.feed([9], [x[:0]], True)[0]                                      # a clip without samples: two frames of zeros
    assert z.shape == (2, 80) and (z == -10.0).all()


def test_64_ragged_clips_in_one_call():
    _need_gpu()
    from sesameai.mel import log_mel
    lens = [1 + (k * 977) % 6000 for k in range(64)]
    clips = [_clip(n, 200 + k) for k, n in enumerate(lens)]
    feats = log_mel(clips, 80)
    for k in (0, 1, 17, 40, 63):
        assert torch.equal(feats[k], _one_shot(clips[k])[1]), k
        assert np.abs(feats[k].cpu().numpy().astype(np.float64) - R.log_mel(clips[k].numpy(), 80)).max() <= 2 * _fixture()["E"]


def test_the_cap_drops_what_comes_after_30_seconds():
    _need_gpu()
    p = _pool(64, 80)
    i = [k for k, g in enumerate(R.GOLDEN_INPUTS) if g[2] == 481000][0]
    x = torch.from_numpy(_input(i)[0])
    assert x.shape[0] == 481000
    p.reset([0, 1, 2])
    full, capped = p.feed([0, 1], [x, x[:480000]], False)
    assert full.shape == (3000, 80) and torch.equal(full, capped) and p.dropped(0) == 1000 and p.dropped(1) == 0
    assert torch.equal(p.finish([full])[0].cpu(), _input(i)[2])
    rows = []
    for a, b in [(0, 479000), (479000, 479999), (479999, 480001), (480001, 480500), (480500, 481000)]:
        rows.append(p.feed([2], [x[a:b]], False)[0].clone())
    assert torch.equal(torch.cat(rows), full) and p.dropped(2) == 1000 and p.frame_count(2, 100, True) == 0
    p.feed([0, 1, 2], [x[:0]] * 3, True)
    assert p.dropped(2) == 0


def test_non_finite_samples_stay_in_their_clip():
    _need_gpu()
    p = _pool(64, 80)
    x, y = _clip(4000, 51), _clip(3333, 52)
    rx, _ = _one_shot(x)
    ry, _ = _one_shot(y)
    bad = x.clone()
    bad[777], bad[2500] = float("nan"), float("inf")
    p.reset([4, 5, 6])
    out = p.feed([4, 5, 6], [x, bad[:3000], y], False)
    assert torch.equal(out[0], rx[:out[0].shape[0]]) and torch.equal(out[2], ry[:out[2].shape[0]])
    assert not torch.isfinite(out[1]).all()
    out = p.feed([5, 4, 6], [bad[3000:], x[:0], y[:0]], True)
    assert torch.equal(torch.cat([rx[:R.frames_needed(4000, False)], out[1]]), rx)
    assert torch.equal(p.feed([5], [y], True)[0], ry)                       # the stream's next clip
    feats = p.finish([rx, torch.full((10, 80), float("nan"), device=rx.device), ry])
    assert torch.equal(feats[0], _one_shot(x)[1]) and torch.equal(feats[2], _one_shot(y)[1])


def test_refusals_leave_the_state_unmoved():
    _need_gpu()
    from sesameai._abi import CsmError
    from sesameai.mel import MelPool
    p = _pool(64, 80)
    x = _clip(5000, 41)
    rx, _ = _one_shot(x)
    p.reset([8])
    a = p.feed([8], [x[:2000]], False)[0].clone()
    for ids, chunks in (([8, 8], [x[:5], x[:5]]), ([64], [x[:5]]), ([-1], [x[:5]]), ([], [])):
        with pytest.raises(CsmError):
            p.feed(ids, chunks, False)
    with pytest.raises(CsmError):
        p.reset([8, 64])
    with pytest.raises(CsmError):
        p.frame_count(64, 5)
    b = p.feed([8], [x[2000:]], True)[0]
    assert torch.equal(torch.cat([a, b]), rx)
    for n, n_mels in ((0, 80), (65, 80), (4, 64)):
        with pytest.raises(CsmError):
            MelPool(n, n_mels)
    with pytest.raises(CsmError):
        p.finish([torch.zeros((3001, 80))])
