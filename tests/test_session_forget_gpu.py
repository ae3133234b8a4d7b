"""Forgetting a session's rows in place on the GPU (include/csm_hip.h csm_session_forget; Session.forget; Generator.open_session(on_full="forget")).

The kernel moves bits and rotates keys with separate fp32 multiplies and adds, so the first half compares ``read()`` with ``torch.equal``
against torch on the CPU: rows below ``a`` keep their bits, V rows from ``a`` on are the old rows + d, K rows from ``a`` on are the fp32
rotation of the old bits by -d positions, rounded once to bf16.  The second half runs endless conversations on the decisive copy
checkpoints, greedy: every turn's codes equal the ANALYTIC trajectory (oracle.csm_ref.decisive_copy_expected_codes) of the trimmed prompt,
which this file derives from the documented policy on its own; the rows that ran are the suffix, so a silent cold fallback fails."""
import ctypes

import pytest
import torch

from test_sessions_gpu import LAG, N, PAGE, ROWS, _cap, _generator, _need_gpu, _restore, _tiny_copy_model, _tiny_model

pytestmark = pytest.mark.gpu


def _unrope(k, d, flavor):
    """K rows [..., hd] bf16 rotated BACK by d positions: fp32 on the bf16 values, products and sums apart, one rounding."""
    from sesameai.models import llama3_rope_theta
    ang = float(d) * llama3_rope_theta(flavor).double()
    c, s = torch.cos(ang).float(), torch.sin(ang).float()
    x = k.float().unflatten(-1, (-1, 2))
    x0, x1 = x[..., 0], x[..., 1]
    return torch.stack([x0 * c + x1 * s, x1 * c - x0 * s], dim=-1).flatten(-2).to(torch.bfloat16)


def _edit(rows, a, b, flavor):
    """[L][2][KV][R][hd] without its rows [a, b): what csm_session_forget is defined to leave."""
    out = torch.cat([rows[:, :, :, :a], rows[:, :, :, b:]], dim=3).clone()
    out[:, 0, :, a:] = _unrope(rows[:, 0, :, b:], b - a, flavor)
    return out


@pytest.fixture(scope="module")
def tiny():
    """(a 3-slot tiny handle whose slots hold 40 rows each and a store of 12 8-row pages, the rows of each slot)."""
    _need_gpu()
    m = _tiny_model()
    want = [_cap(m, s, ROWS) for s in range(3)]
    m.open_session_store(12, PAGE)
    return m, want


def _pages(rows):
    return (rows + PAGE - 1) // PAGE


@pytest.mark.parametrize("cuts", [[(8, 16)], [(5, 7)], [(5, 21)], [(3, 23)], [(0, 9)], [(22, 23)], [(5, 7), (2, 12)]],
                         ids=["page_aligned", "same_page", "mid_page_to_mid_page", "to_the_end", "from_0", "last_row", "two_in_a_row"])
def test_forget_equals_torch_bit_for_bit_then_save_and_load(tiny, cuts):
    m, want = tiny
    s = m.open_session()
    m.save_session(s, 0, 23)
    exp = want[0][:, :, :, :23]
    forgets0 = int(m.describe().split("session_forgets=")[1].split(" ")[0])
    for a, b in cuts:
        before = exp
        s.forget(a, b)
        exp = _edit(before, a, b, m.bb)
        got = s.read()
        assert s.rows == exp.shape[3] and s.pages == _pages(s.rows) and f"session_store=1 sessions, {s.pages}/12 pages" in m.describe()
        assert torch.equal(got[:, :, :, :a], before[:, :, :, :a]), f"forget({a}, {b}): a row below {a} changed"
        assert torch.equal(got[:, 1, :, a:], before[:, 1, :, b:]), f"forget({a}, {b}): V rows from {a} on are not the old rows + {b - a}"
        assert torch.equal(got[:, 0, :, a:], exp[:, 0, :, a:]), f"forget({a}, {b}): K rows from {a} on are not torch's fp32 rotation rounded once"
        if b < before.shape[3]:
            assert not torch.equal(exp[:, 0, :, a:], before[:, 0, :, b:]), "the rotation changes nothing: this case shows nothing"
    assert f"session_forgets={forgets0 + len(cuts)} " in m.describe()
    # the session goes on: more rows from another slot, then a load into a third
    R = s.rows
    m.save_session(s, 1, R + 9)
    exp = torch.cat([exp, want[1][:, :, :, R:R + 9]], dim=3)
    assert s.pages == _pages(R + 9) and torch.equal(s.read(), exp)
    m.load_sessions([s], [2])
    got = _cap(m, 2, ROWS)
    assert torch.equal(got[:, :, :, :R + 9], exp) and torch.equal(got[:, :, :, R + 9:], want[2][:, :, :, R + 9:])
    assert torch.equal(_cap(m, 0, ROWS), want[0]) and torch.equal(_cap(m, 1, ROWS), want[1])
    s.close()
    assert "session_store=0 sessions, 0/12 pages" in m.describe()
    _restore(m, [2])


def test_the_freed_pages_go_to_the_next_save_and_both_sessions_read_back(tiny):
    m, want = tiny
    s = m.open_session()
    m.save_session(s, 0, 23)                                   # pages 0, 1, 2
    s.forget(5, 7)                                             # rewritten into 3 fresh pages; 0, 1, 2 return
    assert s.pages == 3 and "session_store=1 sessions, 3/12 pages" in m.describe()
    exp = _edit(want[0][:, :, :, :23], 5, 7, m.bb)
    t = m.open_session()
    m.save_session(t, 1, ROWS)                                 # 5 pages: the 3 just freed among them (9 are free)
    u = m.open_session()
    m.save_session(u, 2, 32)                                   # the last 4: the pool is full
    assert "session_store=3 sessions, 12/12 pages" in m.describe()
    assert torch.equal(s.read(), exp) and torch.equal(t.read(), want[1]) and torch.equal(u.read(), want[2][:, :, :, :32])
    for x in (s, t, u):
        x.close()


def test_refusals_return_their_code_and_leave_the_session_unchanged(tiny):
    from sesameai._abi import CsmError, lib
    from sesameai.models import SessionPoolFull
    m, want = tiny
    s = m.open_session()
    m.save_session(s, 0, 23)
    before = s.read()
    stream = torch.cuda.current_stream().cuda_stream
    rot = (ctypes.c_float * (m.bb.head_dim))(*([1.0, 0.0] * (m.bb.head_dim // 2)))

    def unchanged():
        assert s.rows == 23 and s.pages == 3 and torch.equal(s.read(), before) and "session_store=" in m.describe()

    for a, b in ((-1, 4), (3, 24), (24, 25), (7, 5)):          # outside [0, rows], to < from
        with pytest.raises(CsmError) as e:
            s.forget(a, b)
        assert e.value.code == -1, str(e.value)
        unchanged()
    used = m.describe().split("session_store=")[1].split(";")[0]
    s.forget(9, 9)                                             # from == to: accepted, nothing happens
    unchanged()
    assert m.describe().split("session_store=")[1].split(";")[0] == used
    assert lib.csm_session_forget(m._h, s._ptr(), 3, 5, None, stream) == -1          # no rotation table
    unchanged()
    gone = m.open_session()
    m.save_session(gone, 1, 9)
    stale = gone._ptr().value
    gone.close()
    assert lib.csm_session_forget(m._h, ctypes.c_void_p(stale), 1, 2, rot, stream) == -1     # a closed session
    with pytest.raises(ValueError):
        gone.forget(1, 2)
    other = _tiny_model(1)
    other.open_session_store(4, PAGE)
    foreign = other.open_session()
    other.save_session(foreign, 0, 12)
    kept = foreign.read()
    assert lib.csm_session_forget(m._h, foreign._ptr(), 1, 2, rot, stream) == -1             # a session of another handle
    assert foreign.rows == 12 and torch.equal(foreign.read(), kept)
    unchanged()
    big = m.open_session()
    m.save_session(big, 1, ROWS)                               # 5 pages, and 2 more below: 10 of 12 held, 2 free
    pad = m.open_session()
    m.save_session(pad, 2, 16)
    with pytest.raises(SessionPoolFull):
        s.forget(5, 7)                                         # needs 3 fresh pages
    unchanged()
    assert "session_store=3 sessions, 10/12 pages" in m.describe()
    s.forget(9, 10)                                            # needs 2: exactly what is free
    assert s.rows == 22 and torch.equal(s.read(), _edit(before, 9, 10, m.bb)) and torch.equal(big.read(), want[1]) and torch.equal(pad.read(), want[2][:, :, :, :16])
    for x in (s, big, pad, foreign):
        x.close()


def test_csm1b_geometry_64_row_pages_1334_rows():
    """CSM-1B cache geometry (16 layers, 8 kv heads, head_dim 64) with 64-row pages: forget [190, 490) and [190, 200) of 1,334 rows."""
    _need_gpu()
    import bench
    from types import SimpleNamespace
    from sesameai.models import Model, csm_1b_args
    a = SimpleNamespace(ctx_text=40, ctx_frames=125, gen_text=24)
    m = Model(csm_1b_args(), None, max_frames=8, max_prefill_rows=2048)
    m.setup_caches(2)
    m.reset_caches()
    S = 1334
    t, mk = bench.synthetic_prompt(a, 1, 128_256, seed0=5000, segments=10, ctx_text=30, ctx_frames=100)
    assert t.shape[1] == S
    m.refill_slot(0, t[0], mk[0], 1.0, 1)
    t1, mk1 = bench.synthetic_prompt(a, 1, 128_256, seed0=5001, segments=10, ctx_text=30, ctx_frames=100)
    m.refill_slot(1, t1[0], mk1[0], 1.0, 1)
    want0 = _cap(m, 0, S)
    m.open_session_store(40, 64)
    for lo, hi in ((190, 490), (190, 200)):
        s = m.open_session()
        m.save_session(s, 0, S)
        assert s.pages == 21
        s.forget(lo, hi)
        exp = _edit(want0, lo, hi, m.bb)
        got = s.read()
        assert s.rows == S - (hi - lo) and s.pages == (s.rows + 63) // 64 and f"session_store=1 sessions, {s.pages}/40 pages" in m.describe()
        assert torch.equal(got[:, :, :, :lo], want0[:, :, :, :lo]) and torch.equal(got[:, 1, :, lo:], want0[:, 1, :, hi:])
        assert torch.equal(got[:, 0, :, lo:], exp[:, 0, :, lo:]) and not torch.equal(exp[:, 0, :, lo:], want0[:, 0, :, hi:])
        m.load_sessions([s], [1])
        assert torch.equal(_cap(m, 1, s.rows), exp) and torch.equal(_cap(m, 0, S), want0)
        s.close()


# ----------------------------------------------------------------------------------------
# endless conversations on the tiny decisive copy checkpoint (lag 20), greedy
# ----------------------------------------------------------------------------------------
# Every reply is N = 8 frames (cut at its limit); csm_tiny's window is 256 rows, so a turn fits while its full prompt is below 248 rows.  A
# turn adds 21 rows (the last reply's EOS row, a user segment of 3 + 4 + 1 rows, 4 text rows of the reply, 8 frames).  The expected
# codes are analytic: frame f names the last code of the row 20 back in the TRIMMED prompt -- right after a forget that is a row that the
# kernel moved, so keys left unrotated, rotated by another d, or V landing on another row change the codes.
SEQ = 256


class _Policy:
    """The documented policy, derived here independently of sesameai/sessions.py: the mirror of one conversation as rows; units end after
    every all-zero audio row; before a turn the smallest number of closed units from unit ``pinned`` on is dropped that makes mirror + EOS
    row + new rows < SEQ - limit."""

    def __init__(self, pinned=1):
        self.t, self.m = torch.zeros(0, 33, dtype=torch.long), torch.zeros(0, 33, dtype=torch.bool)
        self.turns, self.pinned, self.dropped_rows, self.forgets = 0, pinned, 0, 0

    def closed_units(self):
        out, at = [], 0
        for r in range(self.t.shape[0]):
            if bool(self.m[r, :32].all()) and not bool(self.m[r, 32]) and not bool(self.t[r].any()):
                out.append((at, r + 1)); at = r + 1
        return out

    def turn(self, new, limit):
        """-> (the full prompt of the turn, (a, b) rows dropped or None)."""
        R, n_new, room = self.t.shape[0], new[0].shape[0], SEQ - limit
        cut = None
        if R + (1 if self.turns else 0) + n_new >= room:
            units = self.closed_units()
            for n in range(1, len(units) - self.pinned + 1):
                a, b = units[self.pinned][0], units[self.pinned + n - 1][1]
                if R - (b - a) + 1 + n_new < room:
                    cut = (a, b)
                    break
            assert cut is not None, "the dialogue of this test always fits after a forget"
            self.t, self.m = torch.cat([self.t[:cut[0]], self.t[cut[1]:]]), torch.cat([self.m[:cut[0]], self.m[cut[1]:]])
            self.dropped_rows += cut[1] - cut[0]; self.forgets += 1
        eos_t, eos_m = torch.zeros(1, 33, dtype=torch.long), torch.tensor([[True] * 32 + [False]])
        parts_t = [self.t] + ([eos_t] if self.turns else []) + [new[0].long()]
        parts_m = [self.m] + ([eos_m] if self.turns else []) + [new[1].bool()]
        return (torch.cat(parts_t), torch.cat(parts_m)), cut

    def reply(self, full, codes):
        ft = torch.zeros(codes.shape[0], 33, dtype=torch.long); ft[:, :32] = codes.long()
        fm = torch.zeros(codes.shape[0], 33, dtype=torch.bool); fm[:, :32] = True
        self.t, self.m = torch.cat([full[0], ft]), torch.cat([full[1], fm])
        self.turns += 1


def _news(c, turns, voice_frames):
    """Conversation c: per turn the NEW rows (tokens, mask): turn 1 brings the voice prompt (5 text rows, ``voice_frames`` audio rows, EOS)."""
    from oracle import csm_ref as C
    shape = C.csm_tiny()
    g = torch.Generator().manual_seed(900 + c)
    ids = lambda k: torch.randint(0, shape.text_vocab_size, (k,), generator=g).tolist()
    codes = lambda k: torch.randint(1, 2048, (shape.audio_num_codebooks, k), generator=g)
    out = [C.build_prompt([(ids(5), codes(voice_frames)), (ids(4), None)])]
    for _ in range(turns - 1):
        out.append(C.build_prompt([(ids(3), codes(4)), (ids(4), None)]))
    return out


def _expected(full):
    from oracle import csm_ref as C
    return C.decisive_copy_expected_codes(C.csm_tiny(), 1234, full[0], full[1], N, LAG).to(torch.int32)


def _window(monkeypatch):
    import sesameai.generator as G
    monkeypatch.setattr(G, "MAX_SEQ_LEN", SEQ)


def _b1_turn(gen, m, conv, pol, new, label):
    """One B = 1 turn of an on_full="forget" conversation, checked against the policy and the analytic codes; returns the cut."""
    held, forgets = conv.rows, conv.forgets
    full, cut = pol.turn(new, N)
    S = full[0].shape[0]
    want = _expected(full)
    got = gen.generate_codes(*new, N, 1.0, 1, session=conv)[:, 0]
    d = cut[1] - cut[0] if cut else 0
    warm = held - d                                            # the rows the pages hold once the forget has run (unless the session went cold)
    assert conv.forgets == forgets + (1 if cut else 0), f"{label}: the conversation forgot {conv.forgets - forgets} times, the policy says {1 if cut else 0}"
    assert torch.equal(conv.tokens[:S], full[0]) and torch.equal(conv.mask[:S], full[1]), f"{label}: the mirror is not the trimmed prompt"
    assert torch.equal(got, want), f"{label}: the codes leave the analytic trajectory of the trimmed prompt"
    pol.reply(full, got)
    return cut, held, warm, S


@pytest.mark.parametrize("dtype", ["bf16", "fp8"])
def test_tiny_batch_1_third_turn_overflows_and_forgets(monkeypatch, dtype):
    _need_gpu()
    _window(monkeypatch)
    m = _tiny_copy_model(1, dtype)
    gen = _generator(m)
    conv, pol = gen.open_session(on_full="forget", pinned=1), _Policy()
    cuts = []
    for k, new in enumerate(_news(0, 4, 199)):                 # a 205-row voice prompt: 209 + 8, 230 + 8, then 238 + 13 >= 248
        cut, held, warm, S = _b1_turn(gen, m, conv, pol, new, f"turn {k}")
        cuts.append(cut)
        assert m.last_prefill_rows == S - warm, f"turn {k}: {m.last_prefill_rows} rows ran, the suffix after the forget has {S - warm}"
        if cut:
            assert cut[0] == 205 and cut[0] <= S - 1 - LAG < warm, "frame 0 does not read a moved row: this case shows nothing"
    assert cuts[:2] == [None, None] and cuts[2] == (205, 218) and cuts[3] is not None
    assert f"session_forgets={pol.forgets} " in m.describe() and conv.evictions == 0


def test_tiny_sixteen_turns_two_units_forgotten_before_each_of_the_last_five(monkeypatch):
    """The conversation of the CPU check: a 26-row voice prompt, 21 rows per turn; from the 12th turn on two units go before every turn."""
    _need_gpu()
    _window(monkeypatch)
    m = _tiny_copy_model(1, "bf16", pages=64)                  # 31 pages held + 26 fresh ones while a forget right after the voice prompt runs
    gen = _generator(m)
    conv, pol = gen.open_session(on_full="forget", pinned=1), _Policy()
    first = None
    news = _news(1, 17, 20)
    for k, new in enumerate(news):
        cut, held, warm, S = _b1_turn(gen, m, conv, pol, new, f"turn {k}")
        assert m.last_prefill_rows == S - warm, f"turn {k}: a silent cold fallback, or rows run twice"
        if cut and first is None:
            first = k
        if cut:
            assert cut == (26, 47), "reply 1 or its successors: 13 + 8 rows, the two oldest unpinned units"
        if k == 15:
            break
    assert first == 11 and pol.forgets == conv.forgets == 5 and conv.turns == 16 and conv.evictions == 0
    assert f"session_forgets={pol.forgets} " in m.describe()
    # a forget by hand, then barge-in: the (prompt rows, frames) that truncate_last uses moved down with the rows
    rows, (a, b) = conv.tokens.shape[0], conv.closed_units()[1]
    conv.forget(1, 1)
    assert conv.tokens.shape[0] == rows - (b - a) and conv.rows == rows - (b - a) - 1
    conv.truncate_last(3)
    assert conv.tokens.shape[0] == rows - (b - a) - (N - 3) == conv.rows and torch.equal(conv.tokens[-3:, :32], conv.replies[-1].t().long())
    pol.t, pol.m = conv.tokens.clone(), conv.mask.clone()
    cut, held, warm, S = _b1_turn(gen, m, conv, pol, news[16], "the turn after the barge-in")
    assert cut is None and m.last_prefill_rows == S - held


def _live(monkeypatch, dtype, beside, group):
    _need_gpu()
    _window(monkeypatch)
    m = _tiny_copy_model(4, dtype, pages=128)
    gen = _generator(m, batch=4)
    gen.refill_beside_the_loop = beside
    gen.refill_row_layers = 40
    assert m.supports_refill_beside_the_loop(4)
    convs = [gen.open_session(on_full="forget", pinned=1) for _ in range(3)]
    pols = [_Policy() for _ in range(3)]
    news = [_news(c, 4, 199 + c) for c in range(3)]
    plain = [_news(7, 1, 30)[0], _news(8, 1, 41)[0]]           # two requests without a session
    sessions = [convs[0], None, convs[1], convs[2], None]
    forgot = 0
    for k in range(4):
        reqs = [news[0][k], plain[0], news[1][k], news[2][k], plain[1]]
        fulls, warm = [], []
        for r, c in zip(reqs, sessions):
            if c is None:
                fulls.append(r); warm.append(0)
                continue
            pol, held = pols[convs.index(c)], c.rows
            full, cut = pol.turn(r, N)
            forgot += cut is not None
            fulls.append(full); warm.append(held - (cut[1] - cut[0]) if cut else held)
            if cut:
                assert cut[0] <= full[0].shape[0] - 1 - LAG < warm[-1], "frame 0 does not read a moved row"
        rows0 = m.prefill_rows_total
        got = gen.generate_codes_continuous(reqs, N, 1.0, 1, sessions=sessions, **group)
        ran = m.prefill_rows_total - rows0
        assert ran == sum(f[0].shape[0] - w for f, w in zip(fulls, warm)), f"turn {k}: {ran} rows ran -- a silent cold fallback, or rows run twice"
        for i, (g, f, c) in enumerate(zip(got, fulls, sessions)):
            assert torch.equal(g, _expected(f)), f"turn {k} request {i} leaves the analytic trajectory of its (trimmed) prompt"
            if c is not None:
                S = f[0].shape[0]
                assert torch.equal(c.tokens[:S], f[0]) and c.rows == S + N - 1
                pols[convs.index(c)].reply(f, g)
        if k == 2:                                             # no sessions at all: the plain requests' frames are the same
            cold = gen.generate_codes_continuous(fulls, N, 1.0, 1, **group)
            assert torch.equal(cold[1], got[1]) and torch.equal(cold[4], got[4])
    assert forgot >= 3 and sum(c.forgets for c in convs) == forgot and f"session_forgets={forgot} " in m.describe()


@pytest.mark.parametrize("beside", [True, False])
@pytest.mark.parametrize("dtype", ["bf16", "fp8"])
def test_tiny_live_batch_of_4_with_plain_requests_through_both_refill_paths(monkeypatch, dtype, beside):
    _live(monkeypatch, dtype, beside, {})


def test_tiny_live_batch_refill_group_of_3(monkeypatch):
    _live(monkeypatch, "bf16", True, {"refill_group": 3})


@pytest.mark.parametrize("pages, other", [(35, True), (31, False)], ids=["evicts_the_idle_session", "goes_cold_itself"])
def test_tiny_a_store_too_small_for_the_fresh_pages(monkeypatch, pages, other):
    """Turn 3's forget rewrites rows [200, 224) into 3 fresh pages while the session holds 30.  With 35 pages and an idle 4-page session
    one page is free: the idle session is evicted and the turn runs warm.  With 31 pages and nobody to evict the session goes cold itself
    and runs the trimmed mirror."""
    _need_gpu()
    _window(monkeypatch)
    m = _tiny_copy_model(1, "bf16", pages=pages)
    gen = _generator(m)
    idle = None
    if other:
        idle = gen.open_session()
        gen.generate_codes(*_news(5, 1, 14)[0], N, 1.0, 1, session=idle)       # 24 + 7 rows: 4 pages
        assert idle.device.pages == 4
    conv, pol = gen.open_session(on_full="forget", pinned=1), _Policy()
    for k, new in enumerate(_news(0, 3, 199)):
        cut, held, warm, S = _b1_turn(gen, m, conv, pol, new, f"turn {k}")
        if k < 2:
            assert cut is None and m.last_prefill_rows == S - held
    assert cut == (205, 218) and held == 237
    if other:
        assert idle.evictions == 1 and idle.rows == 0 and conv.evictions == 0
        assert m.last_prefill_rows == S - (held - 13), "the turn after the eviction did not run warm"
        assert "session_forgets=1 (19 rows moved)" in m.describe()
    else:
        assert conv.evictions == 1 and m.last_prefill_rows == S, "the session did not go cold itself"
        assert "session_forgets=0 " in m.describe()
    assert conv.rows == S + N - 1 and f"session_store={2 if other else 1} sessions, {conv.device.pages}/{pages} pages" in m.describe()


# ----------------------------------------------------------------------------------------
# CSM-1B shapes: tests/golden/csm1b_forget.pt (tools/make_forget_golden.py) -- the s1334 copy checkpoint (copy layer 3, lag 700)
# ----------------------------------------------------------------------------------------
# Turn 1 is the 1,334-row prompt; then forget_rows(190, 490); turn 2 adds 24 rows.  The golden's codes of turn 2 are the edited-cache
# oracle's = the cold oracle's on the trimmed prompt = the analytic trajectory, with a margin >= 4 x the gap between the two oracles.
@pytest.fixture(scope="module")
def forget1b():
    """(the golden, the checkpoint it was made with): built once for both weight formats."""
    _need_gpu()
    import os
    from test_sessions_gpu import ROOT
    from sesameai.models import csm_1b_args, synthetic_state_dict
    gold = torch.load(os.path.join(ROOT, "tests", "golden", "csm1b_forget.pt"))
    sd = synthetic_state_dict(csm_1b_args(), seed=int(gold["weight_seed"]), flavour=gold["flavour"])
    names, sums = gold["weight_checksums"]
    assert torch.equal(torch.stack([sd[k].view(torch.int16).to(torch.int64).sum() for k in names]), sums), "not the checkpoint the oracle's codes were generated with"
    return gold, sd


@pytest.mark.parametrize("dtype", ["bf16", "fp8"])
def test_csm1b_forget_rows_190_490_then_the_next_turn_equals_the_golden(forget1b, dtype):
    from test_sessions_gpu import _EOS_ROW, _s1334
    from sesameai.models import Model, csm_1b_args
    gold, sd = forget1b
    g = gold[dtype]
    assert g["margin"] >= 4 * g["gap"] and tuple(gold["forget"]) == (190, 490) and int(gold["lag"]) == 700
    first, n = _s1334(), int(gold["frames"])
    assert first[0].shape[0] == int(gold["prompt_rows"]) == 1334
    m = Model(csm_1b_args(), sd, max_frames=32, max_prefill_rows=2048, weights_dtype=dtype)
    m.setup_caches(1)
    m.open_session_store(48, 64)
    gen = _generator(m)
    conv = gen.open_session()
    codes1 = g["codes1"].to(torch.int32)
    assert torch.equal(gen.generate_codes(*first, n, 1.0, 1, session=conv)[:, 0], codes1), "turn 1 differs from the golden"
    assert conv.rows == 1334 + n - 1 and conv.device.pages == 21
    conv.forget_rows(190, 490)
    held = 1334 + n - 1 - 300
    assert conv.rows == held == int(g["held2"]) and conv.tokens.shape[0] == 1334 + n - 300 and conv.device.pages == (held + 63) // 64
    assert "session_forgets=1 " in m.describe()
    new = gold["new_tokens"].long(), gold["new_mask"]
    S2 = int(g["full_rows2"])
    assert S2 == held + 1 + 1 + new[0].shape[0] and 190 <= S2 - 1 - 700 < held, "frame 0 does not read a moved row"
    ft = torch.zeros(n, 33, dtype=torch.long); ft[:, :32] = codes1.long()
    trimmed = torch.cat([first[0][:190], first[0][490:], ft, _EOS_ROW[0], new[0]])
    got = gen.generate_codes(*new, n, 1.0, 1, session=conv)[:, 0]
    assert m.last_prefill_rows == S2 - held, f"{m.last_prefill_rows} rows ran, the suffix after the forget has {S2 - held}"
    assert torch.equal(conv.tokens[:S2], trimmed), "the mirror is not the trimmed prompt"
    want = g["codes2"].to(torch.int32)
    assert torch.equal(got, want), f"turn 2 leaves the golden at frame {int((got != want).any(dim=1).nonzero()[0]) if got.shape == want.shape else got.shape}"
    paths = m.fast_paths()
    assert paths & 1 and paths & 32 and paths & (16 if dtype == "fp8" else 8), f"k_bb_layer, k_dec_first or k_dec_persist was off: {paths}"
    conv.close()
