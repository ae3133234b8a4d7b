"""Host logic of the endless conversations (no GPU): ``Generator.open_session(on_full="forget")`` on scripted models (tests/test_sessions_host_logic.py)
that also record ``Session.forget``.  Checked: the unit split; that pinned units, the open unit and the new rows are never dropped and the
number dropped is the smallest that fits; the ValueError when nothing fits; the order forget -> load -> prefill / refill with one load per
refill group; that the rows run are the suffix after the forget; ``truncate_last`` after a forget; a pool too short for the fresh pages
(the least recently used conversation outside the call is evicted, else the session goes cold itself); a cold session trims only its
mirror; and that on_full="raise" or no session shows the model no forget and raises today's ValueError."""
import pytest
import torch

from test_host_logic import _FakeCodec, _scripted
from test_prefix_host_logic import _rows, _scripts
from test_sessions_host_logic import EOS_ROW, PAGE, _BesideS, _cat, _check_turn, _Dev, _GroupS, _One, _SlotsS, _audio_rows

SEQ, LIMIT = 96, 6            # the window of these tests (sesameai.generator.MAX_SEQ_LEN is patched) and every reply's length limit: room for 89 rows


class _DevF(_Dev):
    """``_Dev`` plus ``Session.forget``: rows from a // PAGE * PAGE on go to fresh pages before the old ones return."""

    def forget(self, a, b):
        from sesameai.models import SessionPoolFull
        assert self.alive and 0 <= a < b <= self.rows
        used = sum(d.pages for d in self.model.devs)
        fresh = (self.rows - (b - a) + PAGE - 1) // PAGE - a // PAGE
        if used + fresh > self.model.pool_pages:
            self.model.log.append(("forget_refused", self.sid))
            raise SessionPoolFull("scripted")
        self.model.log.append(("forget", self.sid, a, b))
        self.rows -= b - a


def _forgetting(cls):
    class F(cls):
        def open_session(self):
            dev = super().open_session()
            dev.__class__ = _DevF
            return dev
    return F


_OneF, _SlotsF, _BesideF, _GroupF = _forgetting(_One), _forgetting(_SlotsS), _forgetting(_BesideS), _forgetting(_GroupS)


@pytest.fixture(autouse=True)
def _window(monkeypatch):
    import sesameai.generator as G
    monkeypatch.setattr(G, "MAX_SEQ_LEN", SEQ)


def _frames(n, seed):
    return torch.randint(1, 2048, (n, 32), generator=torch.Generator().manual_seed(seed))


def _segment(ids, n_audio, seed):
    """A context segment's rows: its text, its audio, the all-zero EOS row."""
    return _cat(_rows(ids), _audio_rows(_frames(n_audio, seed)), EOS_ROW)


def _is_eos(t, m, r):
    return bool(m[r, :32].all()) and not bool(m[r, 32]) and not bool(t[r].any())


def _expect(t, m, turns, new, pinned, limit=LIMIT):
    """The documented policy, derived here: -> (the turn's full prompt, the rows (a, b) dropped or None)."""
    closed, at = [], 0
    for r in range(t.shape[0]):
        if _is_eos(t, m, r):
            closed.append((at, r + 1)); at = r + 1
    room, cut = SEQ - limit, None
    if t.shape[0] + (1 if turns else 0) + new[0].shape[0] >= room:
        for n in range(1, len(closed) - pinned + 1):
            a, b = closed[pinned][0], closed[pinned + n - 1][1]
            if t.shape[0] - (b - a) + 1 + new[0].shape[0] < room:
                cut = (a, b)
                break
    if cut:
        t, m = torch.cat([t[:cut[0]], t[cut[1]:]]), torch.cat([m[:cut[0]], m[cut[1]:]])
    return _cat((t, m), *([EOS_ROW] if turns else []), new), cut


def _new(k, pid=0):
    """Turn k's new rows: turn 0 brings a 24-row voice prompt; later turns a 6-row user segment; then 2 text rows of the reply."""
    if k == 0:
        return _cat(_segment([900, 901, 902], 20, 50), _rows([700, pid]))
    return _cat(_segment([800 + k, 810 + k], 3, 60 + k), _rows([700 + k, pid]))


def _b1(pinned=1, turns=5):
    """A conversation of ``turns`` turns at batch 1, every reply cut at LIMIT frames: 26 + 6 rows, then 15 per turn."""
    from sesameai.generator import Generator
    model = _OneF(_scripted(64, 1, [11]))
    gen = Generator(model, audio_tokenizer=_FakeCodec())
    conv = gen.open_session(on_full="forget", pinned=pinned)
    for k in range(turns):
        gen.generate_codes(*_new(k), LIMIT, 0.9, 50, session=conv)
    return gen, model, conv


def test_units_split_after_every_eos_row_and_the_tail_is_open():
    gen, model, conv = _b1(turns=3)
    assert conv.tokens.shape[0] == 62 and conv.rows == 61 and not [e for e in model.log if e[0] == "forget"]
    #          voice     reply 1 + EOS   user 2    reply 2 + EOS   user 3    reply 3 (open)
    units = [(0, 24), (24, 33), (33, 39), (39, 48), (48, 54), (54, 62)]
    assert conv.units() == units and conv.closed_units() == units[:-1]
    assert all(_is_eos(conv.tokens, conv.mask, b - 1) for _, b in units[:-1]) and not _is_eos(conv.tokens, conv.mask, 61)
    fresh = gen.open_session()
    assert fresh.units() == [] and fresh.closed_units() == [] and fresh.on_full == "raise" and fresh.pinned == 1
    with pytest.raises(ValueError):
        gen.open_session(on_full="drop")
    with pytest.raises(ValueError):
        gen.open_session(on_full="forget", pinned=-1)
    with pytest.raises(ValueError):
        conv.forget(4, 2)                                       # unit 5 is the open one


@pytest.mark.parametrize("pinned, cut", [(1, (24, 39)), (2, (33, 48)), (0, (0, 24)), (4, (48, 63))])
def test_batch_1_drops_the_smallest_number_of_units_after_the_pinned_ones_then_loads_then_runs_the_suffix(pinned, cut):
    gen, model, conv = _b1(pinned)
    assert conv.tokens.shape[0] == 92 and conv.rows == 91 and conv.forgets == 0        # turn 6 would need 92 + 1 + 8 rows: 89 fit
    t0, m0 = conv.tokens.clone(), conv.mask.clone()
    full, want_cut = _expect(t0, m0, 5, _new(5), pinned)
    assert want_cut == cut
    for n in range(1, 6):                                      # the count is the smallest: one unit fewer does not fit
        a, b = conv.closed_units()[pinned][0], conv.closed_units()[min(pinned + n, 9) - 1][1]
        if b == cut[1]:
            break
        assert 92 - (b - a) + 1 + 8 >= SEQ - LIMIT
    d = cut[1] - cut[0]
    del model.log[:]
    gen.generate_codes(*_new(5), LIMIT, 0.9, 50, session=conv)
    assert model.log[:4] == [("forget", 0, *cut), ("reset_caches",), ("load", [0], [0], [91 - d]), ("prefill_prompt", 101 - d, 91 - d)], model.log[:4]
    assert len([e for e in model.log if e[0] == "forget"]) == 1 and conv.forgets == 1
    assert torch.equal(model.prompts[-1][0], full[0]) and torch.equal(model.prompts[-1][1], full[1]), "the prompt is not the trimmed one"
    kept = torch.cat([t0[:cut[0]], t0[cut[1]:]])
    assert torch.equal(full[0][:92 - d], kept) and torch.equal(full[0][-8:], _new(5)[0]), "only rows of whole units after the pinned ones went"
    assert torch.equal(full[0][:conv.closed_units()[pinned][0]], t0[:cut[0]]), "a pinned unit was touched"
    assert torch.equal(full[0][92 - d - 8:92 - d], t0[84:]), "the open unit (reply 5) was touched"
    assert model.log[-1] == ("save", 0, 0, 91 - d, 101 - d + LIMIT - 1) and conv.tokens.shape[0] == 101 - d + LIMIT


def test_nothing_fits_is_todays_value_error_and_nothing_is_dropped():
    gen, model, conv = _b1()
    t0 = conv.tokens.clone()
    del model.log[:]
    big = _cat(_segment([1, 2], 60, 9), _rows([3, 0]))          # 24 pinned + 8 open + 1 + 65 new rows >= 90 whatever goes
    with pytest.raises(ValueError, match="Inputs too long, must be below max_seq_len - max_generation_len: 90"):
        gen.generate_codes(*big, LIMIT, 0.9, 50, session=conv)
    with pytest.raises(ValueError, match="Inputs too long"):
        list(gen.generate_stream([5] * 70, 0, [], max_audio_length_ms=LIMIT * 80, session=conv))
    assert model.log == [] and torch.equal(conv.tokens, t0) and conv.rows == 91 and conv.forgets == 0
    assert conv.plan_forget(65, LIMIT, SEQ) == (1, 0) and conv.plan_forget(8, LIMIT, SEQ) == (1, 2) and conv.plan_forget(8, 3, SEQ) == (1, 1)
    assert conv.plan_forget(1, 1, SEQ) == (1, 0) and conv.plan_forget(2, 1, SEQ) == (1, 1), "92 + 1 + 1 rows fit below 95, one more does not"


def test_on_full_raise_and_no_session_show_the_model_no_forget():
    from sesameai.generator import Generator
    model = _OneF(_scripted(64, 1, [11]))
    gen = Generator(model, audio_tokenizer=_FakeCodec())
    conv = gen.open_session()                                   # on_full="raise"
    for k in range(5):
        gen.generate_codes(*_new(k), LIMIT, 0.9, 50, session=conv)
    del model.log[:]
    with pytest.raises(ValueError, match="Inputs too long, must be below max_seq_len - max_generation_len: 90"):
        gen.generate_codes(*_new(5), LIMIT, 0.9, 50, session=conv)
    assert model.log == [] and conv.tokens.shape[0] == 92 and conv.rows == 91
    with pytest.raises(ValueError, match="Inputs too long"):
        gen.generate_codes(*_rows(list(range(90))), LIMIT, 0.9, 50)
    gen.generate_codes(*_new(1), LIMIT, 0.9, 50)
    assert model.log[:2] == [("reset_caches",), ("prefill_prompt", 8, None)] and not [e for e in model.log if e[0] in ("forget", "load", "save")]


def test_truncate_last_after_a_forget_cuts_the_right_rows():
    gen, model, conv = _b1()
    gen.generate_codes(*_new(5), LIMIT, 0.9, 50, session=conv)  # forgets [24, 39): full prompt 86 rows, 6 frames
    frames = model.frames[:, 0]
    assert conv.tokens.shape[0] == 92 and conv.rows == 91 and conv._last == (86, 6)
    del model.log[:]
    conv.forget(1, 1)                                           # by hand, AFTER the turn: reply 2 + its EOS row, 9 rows
    assert model.log == [("forget", 0, 24, 33)] and conv._last == (77, 6) and conv.rows == 82 and conv.tokens.shape[0] == 83
    conv.truncate_last(2)
    assert model.log[-1] == ("truncate", 0, 79) and conv.rows == 79 == conv.tokens.shape[0]
    assert torch.equal(conv.tokens[77:, :32], frames[:2].long()) and conv.replies[-1].shape == (32, 2)
    with pytest.raises(ValueError):
        conv.forget_rows(70, 78)                                # into the last reply's frames
    t0, m0 = conv.tokens.clone(), conv.mask.clone()
    full, cut = _expect(t0, m0, 6, _new(6), 1)
    assert cut is None
    del model.log[:]
    gen.generate_codes(*_new(6), LIMIT, 0.9, 50, session=conv)
    assert model.log[:3] == [("reset_caches",), ("load", [0], [0], [79]), ("prefill_prompt", 88, 79)]
    assert torch.equal(model.prompts[-1][0], full[0]) and torch.equal(model.prompts[-1][1], full[1])


def test_a_pool_too_short_evicts_the_lru_conversation_outside_the_call_else_the_session_goes_cold_itself():
    from sesameai.generator import Generator
    model = _OneF(_scripted(64, 1, [11]))
    gen = Generator(model, audio_tokenizer=_FakeCodec())
    idle = gen.open_session()
    gen.generate_codes(*_new(0), LIMIT, 0.9, 50, session=idle)  # 26 + 5 rows: 4 pages; used before all of conv's turns: the least recently used
    conv = gen.open_session(on_full="forget")
    for k in range(5):
        gen.generate_codes(*_new(k), LIMIT, 0.9, 50, session=conv)
    assert conv.rows == 91 and conv.device.pages == 12 and idle.device.pages == 4
    model.pool_pages = 12 + 4 + 4                               # 4 free; the forget of [24, 39) rewrites rows [24, 76): 10 - 3 = 7 fresh pages
    del model.log[:]
    full, cut = _expect(conv.tokens.clone(), conv.mask.clone(), 5, _new(5), 1)
    assert cut == (24, 39)
    gen.generate_codes(*_new(5), LIMIT, 0.9, 50, session=conv)
    assert model.log[:6] == [("forget_refused", 1), ("truncate", 0, 0), ("forget", 1, 24, 39), ("reset_caches",), ("load", [1], [0], [76]), ("prefill_prompt", 86, 76)]
    assert idle.evictions == 1 and idle.rows == 0 and idle.tokens.shape[0] == 32 and conv.evictions == 0
    assert torch.equal(model.prompts[-1][0], full[0])
    # nobody left to evict: the session goes cold itself and runs its TRIMMED mirror whole
    assert conv.rows == 91 and conv.tokens.shape[0] == 92
    model.pool_pages = 12 + 3
    del model.log[:]
    full, cut = _expect(conv.tokens.clone(), conv.mask.clone(), 6, _new(6), 1)
    assert cut == (24, 39)
    gen.generate_codes(*_new(6), LIMIT, 0.9, 50, session=conv)
    assert model.log[:4] == [("forget_refused", 1), ("truncate", 1, 0), ("reset_caches",), ("prefill_prompt", 86, None)]
    assert conv.evictions == 1 and torch.equal(model.prompts[-1][0], full[0]) and not [e for e in model.log if e[0] in ("load", "forget")]
    # a cold session trims only its mirror
    idle2 = gen.open_session(on_full="forget")
    idle2.tokens, idle2.mask, idle2.turns, idle2._last = conv.tokens.clone(), conv.mask.clone(), conv.turns, conv._last
    del model.log[:]
    rows = idle2.tokens.shape[0]
    idle2.forget(1, 2)
    assert model.log == [] and idle2.rows == 0 and idle2.tokens.shape[0] < rows and idle2.forgets == 1


@pytest.mark.parametrize("model_cls, group", [(_SlotsF, 1), (_BesideF, 1), (_GroupF, 4)])
def test_live_batch_forgets_before_the_loads_and_runs_only_the_suffixes(model_cls, group):
    from sesameai.generator import Generator
    lens = [7, 9, 3, 8, 6, 10, 2, 7, 9, 6, 5, 8]                # requests 0..3: turn 1, 4..7: turn 2, 8..11: turn 3; request 4k + 2 is plain
    scripts = _scripts(lens, 31)
    model = model_cls(scripts, 3)
    gen = Generator(model, audio_tokenizer=_FakeCodec(), max_batch_size=3)
    gen.refill_row_layers = 40
    convs = [gen.open_session(on_full="forget", pinned=1) for _ in range(3)]
    sessions = [convs[0], convs[1], None, convs[2]]
    kw = {"refill_group": group} if group > 1 else {}

    def news(k):
        out = []
        for j in range(4):
            pid = 4 * k + j
            if k == 0 and j != 2:                              # a 64-row voice prompt: 66 + 6, + 15, and turn 3 overflows
                out.append(_cat(_segment([900 + j, 901], 61, 40 + j), _rows([700, pid])))
            elif j == 2:
                out.append(_rows([300 + k, 301, pid]))
            else:
                out.append(_cat(_segment([800 + k, 810 + j], 3, 60 + pid), _rows([700 + k, pid])))
        return out

    for k in range(3):
        reqs = news(k)
        full, held, cuts = [], [], []
        for r, c in zip(reqs, sessions):
            if c is None:
                full.append(r); held.append(0); cuts.append(None)
                continue
            f, cut = _expect(c.tokens.clone(), c.mask.clone(), c.turns, r, 1)
            full.append(f); cuts.append(cut); held.append(c.rows - (cut[1] - cut[0] if cut else 0))
        del model.log[:]
        out = gen.generate_codes_continuous(reqs, LIMIT, 0.9, 50, sessions=sessions, **kw)
        log = list(model.log)
        forgets = [e for e in log if e[0] == "forget"]
        assert forgets == [("forget", c.device.sid, *cut) for c, cut in zip(sessions, cuts) if cut], f"turn {k}: {forgets}"
        assert log[:len(forgets)] == forgets, "a forget is enqueued ahead of every load and refill of its call"
        assert (len(forgets) == 3) == (k == 2)
        for c, f in zip(sessions, full):
            if c is not None:
                S = f[0].shape[0]
                assert torch.equal(c.tokens[:S], f[0]) and torch.equal(c.mask[:S], f[1]), "the mirror is not the trimmed prompt + the reply"
        _check_turn(model_cls, lens, LIMIT, sessions, full, held, log[len(forgets):], out, scripts, list(range(4 * k, 4 * k + 4)))
    assert cuts[0] == (64, 73) and all(c.forgets == 1 and c.turns == 3 for c in convs)
    if group > 1:
        assert max(len(e[1]) for e in log if e[0] == "load") >= 2, "several sessions of one group share one load"
    # a request that cannot fit leaves EVERY session of the call as it was
    del model.log[:]
    rows = [c.tokens.shape[0] for c in convs]
    with pytest.raises(ValueError, match="Inputs too long"):
        gen.generate_codes_continuous([news(1)[0], news(1)[1], _rows(list(range(95))), news(1)[3]], LIMIT, 0.9, 50, sessions=sessions, **kw)
    assert model.log == [] and [c.tokens.shape[0] for c in convs] == rows
