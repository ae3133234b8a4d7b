"""The leveler's rule on its own (tests/leveler_ref.py; include/mimi_hip.h, mimi_ld_pool_level_*), no GPU: it holds nothing back, a stream
over any chunk schedule is the one-shot result, a small ring is seen, the gain law's exact property, and what it does to the meter
tests' own inputs at -19 LUFS under a -1 dBFS ceiling.  The bound of 0.5 LU covers the moving integrated estimate the gain follows
after it has reached its target -- the rule gave 0.001 (sine), 0.13 and 0.06 LU there -- not device error: the device has none."""
import numpy as np
import pytest

import leveler_ref as R
import loudness_ref as L
from test_loudness_oracle import clip, plosive, sine, speechlike

P = R.params(-19.0)
BOUND = 0.5                 # LU
_made = {}


def levelled(name, p=P, ring=L.RING):
    make = {"speech 20 s": lambda: speechlike(20.0, 0.9), "speech 12 s": lambda: speechlike(12.0, 0.3, 5), "sine": lambda: sine(1000.0, 8.0, -6.0),
            "quiet": lambda: speechlike(20.0, 0.05), "plosive": plosive}
    if name not in _made:
        _made[name] = make[name]()
    key = (name, p, ring)
    if key not in _made:
        _made[key] = R.level_ref(_made[name], p, ring)
    return _made[name], _made[key]


def test_the_defaults():
    assert P == R.Params(L.target_ms(-19.0), L.ceiling_i16(-1.0), 65536, 16 * 65536, 4) and P.C == 29203
    assert R.params(-19.0, max_gain_db=12.0).gmax == 4 * 65536 and R.params(-19.0, start_gain=0.5).g0 == 32768
    for bad in (dict(start_gain=0.0), dict(start_gain=17.0), dict(max_gain_db=37.0), dict(slew_shift=0), dict(slew_shift=17)):
        with pytest.raises(AssertionError):
            R.params(-19.0, **bad)


@pytest.mark.parametrize("kind", ["fp32", "int16"])
@pytest.mark.parametrize("N", [0, 1, 2399, 2400, 2401, 9600, 24007, 60001])
def test_stream_equals_one_shot_and_nothing_is_held_back(N, kind):
    x = np.concatenate([clip("speech 0.9")[3000:40000], clip("square 3 kHz")])[:N]
    x = x if kind == "fp32" else L.to_s(x).astype(np.int16)
    p = R.params(-23.0, ceiling_db=-3.0)
    want = R.level_ref(x, p)
    assert want.y.shape == x.shape and want.y.dtype == x.dtype and want.gains.shape[0] == N // L.H + 2
    schedules = {"inside a hop": [1000, 3000, 700], "on the hop edges": [2400, 2400, 4800], "around them": [1, 2399, 2400, 2401, 511, 0],
                 "frames": [3840] + [1920] * 40, "sample by sample over an edge": [2398, 1, 1, 1, 1]}
    for name, steps in schedules.items():
        st = R.LevelerRef(p)
        ys, es, gs, a = [], [], [], 0
        for c in steps + [N]:
            c = min(c, N - a)
            y, e, g = st.feed(x[a:a + c])
            assert y.shape[0] == c and g.shape[0] == e.shape[0] + 2                # n_out == n_in on every call
            ys.append(y); es.append(e); gs.append(g if not gs else g[2:])
            a += c
        y, e, g = st.feed(x[:0], final=True)                                       # an empty chunk closes the clip
        assert y.shape[0] == 0 and e.shape[0] == 0 and np.array_equal(g, want.gains[-2:])
        assert np.array_equal(np.concatenate(ys), want.y, equal_nan=True) and np.array_equal(np.concatenate(es), want.energies), (N, name)
        assert np.array_equal(np.concatenate(gs), want.gains) and st.row == want.row, (N, name)
        assert (st.R, st.k, st.clipped, st.a_next) == (0, 0, 0, p.g0)              # fresh, with the same parameters
        y2 = st.feed(x, final=True)[0]
        assert np.array_equal(y2, want.y, equal_nan=True) and st.row == want.row, "the next clip on the same stream"


def test_final_levels_the_trailing_partial_hop():
    x = clip("speech 0.9")[:2400 * 12 + 1700]
    st = R.LevelerRef(P)
    y = st.feed(x, final=True)[0]
    w = R.level_ref(x, P)
    assert np.array_equal(y, w.y) and y.shape[0] == x.shape[0]
    gi = R.sample_gains(w.gains, 2400 * 12, 1700)                                  # between A[12] and A[13], both known before the hop began
    assert gi[0] == w.gains[12] and np.array_equal(y[2400 * 12:], R.apply_gains(x[2400 * 12:], gi, P.C)[0])


def test_a_ring_of_8_over_25_hops():
    x = clip("loud then quiet")[60000:120000]
    w8, w = R.level_ref(x, P, 8), R.level_ref(x, P)
    assert len(w8.energies) == 25 and not np.array_equal(w8.gains, w.gains) and np.array_equal(w8.gains[:10], w.gains[:10])
    e, pk = [int(v) for v in w8.energies], R.hop_peaks(L.to_s(x))
    for j in range(1, 26):                                                         # every boundary from the last 8 hops alone
        S, n = L.gate(e[max(0, j - 8):j], 8)
        assert w8.gains[j + 1] == R.next_gain(int(w8.gains[j]), S, n, int(pk[:j].max()), P)[0]
    st = R.LevelerRef(P, ring=8)
    ys = [st.feed(x[a:b])[0] for a, b in ((0, 31000), (31000, 40000), (40000, 60000))]
    assert np.array_equal(np.concatenate(ys), w8.y) and st.row == w8.row


@pytest.mark.parametrize("name", ["speech 20 s", "speech 12 s", "sine", "quiet", "plosive"])
def test_once_the_slew_no_longer_binds_the_gain_is_the_target_under_its_caps(name):
    """the exact property: |T - A[j]| <= d  =>  A[j + 1] == min(T, cap, gmax); and otherwise the gain moves by exactly d towards T,
    unless a cap stops it"""
    _, w = levelled(name)
    A, seen = w.gains, set()
    for j, T, d, cap in w.trace:
        if T is None:
            assert A[j + 1] == max(1, min(A[j], cap, P.gmax))
        elif abs(T - A[j]) <= d:
            assert A[j + 1] == max(1, min(T, cap, P.gmax))
            seen.add("reached")
        else:
            assert A[j + 1] == max(1, min(A[j] + d if T > A[j] else A[j] - d, cap, P.gmax))
            seen.add("slewing")
        assert 1 <= A[j + 1] <= min(cap, P.gmax) and d == max(1, A[j] >> P.sh)
    assert "slewing" in seen


@pytest.mark.parametrize("name,hop,lu", [("speech 20 s", 9, 0.13), ("speech 12 s", 21, 0.06), ("sine", 22, 0.001)])
def test_the_output_measures_its_target_from_where_the_gain_reached_it(name, hop, lu):
    x, w = levelled(name)
    j = R.reach(w.gains, w.trace, P)
    got = R.lufs_after(w.y, j)
    print(f"{name}: reaches its target gain at hop {j}; measures {got:.3f} LUFS from there on ({L.lufs(*L.measure_ref(x)[:2]):.2f} LUFS in)")
    assert j == hop and abs(got + 19.0) <= BOUND and abs(abs(got + 19.0) - lu) < 0.01
    assert w.row[2] == 0 and np.abs(w.y).max() <= np.float32(P.C) / 32768


def test_the_quiet_clip_ends_on_gmax():
    x, w = levelled("quiet")
    first = int(np.argmax(w.gains == P.gmax))
    S, n = L.measure_ref(w.y)[:2]
    print(f"quiet: {L.lufs(*L.measure_ref(x)[:2]):.2f} LUFS in; on gmax from hop {first}; ends {-19.0 - L.lufs(S, n):.2f} LU low")
    assert w.gains[-1] == P.gmax == w.row[0] and first == 50 and (w.gains[first:] == P.gmax).all()
    assert 0.5 < -19.0 - L.lufs(S, n) < 1.5                                        # the known limit: 24 dB are not enough for -44 LUFS


def test_the_plosive_is_held_by_the_cap_and_clamped():
    x, w = levelled("plosive")
    s = L.to_s(w.y)
    print(f"plosive: {w.row[2]} samples clamped; the gain ends on {w.row[0] / 65536:.4f}; peak in {w.row[3]}, out {int(np.abs(s).max())}")
    assert w.row[2] == 18 and int(np.abs(s).max()) <= P.C and np.abs(w.y).max() == np.float32(P.C) / 32768
    after = [(a, cap) for a, (j, T, d, cap) in zip(w.gains[2:], w.trace) if j >= 14]              # the plosive sits in hop 12
    assert all(a <= cap for a, cap in after) and any(a == cap for a, cap in after) and abs(w.row[0] / 65536 - 1.0) < 0.02
    yi = R.level_ref(L.to_s(x).astype(np.int16), P)                                # the int16 path clamps the same samples
    assert yi.row == w.row and int(np.abs(yi.y.astype(np.int64)).max()) == P.C


def test_the_slew_is_seen():
    x, w = levelled("sine")
    slow = R.params(-19.0, slew_shift=8)
    _, w8 = levelled("sine", slow)
    j4, j8 = R.reach(w.gains, w.trace, P), R.reach(w8.gains, w8.trace, slow)
    assert j4 == 22 and (j8 is None or j8 > j4) and not np.array_equal(w.gains, w8.gains)
    assert all(abs(int(b) - int(a)) <= max(1, int(a) >> 8) for a, b in zip(w8.gains[1:], w8.gains[2:]))


def test_nan_inf_and_the_absolute_gate():
    x = clip("speech 0.9")[:30000].copy()
    x[12345], x[12346], x[20000] = np.nan, np.inf, -np.inf
    w = R.level_ref(x, P)
    Cf = np.float32(P.C) / 32768
    assert np.isnan(w.y[12345]) and w.y[12346] == Cf and w.y[20000] == -Cf and w.row[2] >= 2 and np.isfinite(np.delete(w.y, 12345)).all()
    quiet = speechlike(2.0, 1.0, 5) * np.float32(10 ** (-75 / 20))
    wq = R.level_ref(quiet, R.params(-19.0, start_gain=0.5))
    assert set(wq.gains.tolist()) == {32768} and np.array_equal(wq.y, quiet * np.float32(0.5))     # nothing above -70 LUFS: the gain stays g0
