"""Host logic of the conversation sessions (no GPU): scripted models stand in for the frame loop (tests/test_host_logic.py, tests/test_prefix_host_logic.py)
and record the session calls.  What is checked is the bookkeeping of sesameai/sessions.py, Generator._frame_blocks and the live batch
(sesameai/live_batch.py, both refill policies and the group refill): that the load sits immediately in front of the refill / prefill it
belongs to and only the rows after the session's run; that the save comes after the block has been read and before the slot is rewound or
refilled; how many rows are saved (P + n after a sampled EOS, P + n - 1 at the length limit); what the next turn's suffix is; that a session
takes one request per call; eviction; and ``truncate_last``."""
import pytest
import torch

from test_group_refill_host_logic import _Group
from test_host_logic import _FakeCodec, _ScriptedModel, _scripted
from test_prefix_host_logic import _Beside, _Slots, _rows, _scripts

PAGE = 8


class _Dev:
    """Stands in for sesameai.models.Session."""

    def __init__(self, model, sid):
        self.model, self.sid, self.rows, self.alive = model, sid, 0, True

    @property
    def pages(self):
        return (self.rows + PAGE - 1) // PAGE

    def truncate(self, rows):
        assert self.alive and 0 <= rows <= self.rows
        self.model.log.append(("truncate", self.sid, rows))
        self.rows = rows

    def close(self):
        self.rows, self.alive = 0, False


class _SessionCalls:
    """The session surface of sesameai.models.Model on a scripted model: a pool of ``pool_pages`` pages of 8 rows."""
    pool_pages = 1 << 20

    def open_session(self):
        if not hasattr(self, "devs"):
            self.devs = []
        self.devs.append(_Dev(self, len(self.devs)))
        return self.devs[-1]

    def save_session(self, dev, slot, rows):
        from sesameai.models import SessionPoolFull
        assert dev.alive and rows >= dev.rows
        used = sum(d.pages for d in self.devs)
        if used - dev.pages + (rows + PAGE - 1) // PAGE > self.pool_pages:
            self.log.append(("save_refused", dev.sid))
            raise SessionPoolFull("scripted")
        self.log.append(("save", dev.sid, slot, dev.rows, rows))
        dev.rows = rows

    def load_sessions(self, devs, slots):
        assert all(d.alive and d.rows > 0 for d in devs) and len(set(slots)) == len(slots) == len(devs)
        self.log.append(("load", [d.sid for d in devs], list(slots), [d.rows for d in devs]))

    def reset_slots(self, slots):
        self.log.append(("reset_slots", list(slots)))
        super().reset_slots(slots)

    def read_frames(self, B, first=0, n=None):
        self.log.append(("read",))
        return super().read_frames(B, first, n)


class _SlotsS(_SessionCalls, _Slots):
    pass


class _BesideS(_SessionCalls, _Beside):
    pass


class _GroupS(_SessionCalls, _Group):
    pass


class _One(_SessionCalls, _ScriptedModel):
    """The batch-1 loop's model: one script, replayed from its start by every turn."""

    def __init__(self, frames):
        super().__init__(frames)
        self.log, self.prompts = [], []

    def reset_caches(self):
        self.log.append(("reset_caches",))
        super().reset_caches()

    def prefill_prompt(self, t, m, start=None):
        self.log.append(("prefill_prompt", t.shape[1], start))
        self.prompts.append((t[0].clone(), m[0].clone()))
        return t.shape[1] - (start or 0)

    def step(self, B, T, k, use_graph=True):
        self.log.append(("step",))
        super().step(B, T, k, use_graph)


def _audio_rows(frames):
    t = torch.zeros(frames.shape[0], 33, dtype=torch.long); t[:, :32] = frames.long()
    m = torch.zeros(frames.shape[0], 33, dtype=torch.bool); m[:, :32] = True
    return t, m


EOS_ROW = _audio_rows(torch.zeros(1, 32))


def _cat(*parts):
    return torch.cat([p[0] for p in parts], 0), torch.cat([p[1] for p in parts], 0)


def test_batch_1_three_turns_rows_saved_suffix_and_call_order():
    from sesameai.generator import Generator
    script = _scripted(64, 1, [11])                             # every turn: EOS sampled as frame 11 -- unless its limit comes first
    model = _One(script)
    gen = Generator(model, audio_tokenizer=_FakeCodec())
    conv = gen.open_session()
    assert conv.rows == 0 and conv.turns == 0
    frames = script[:, 0]
    new1, new2, new3 = _rows([900 + i for i in range(20)]), _rows([1, 2, 3, 4]), _rows([5, 6, 7])
    # turn 1: cold -- no load, the whole prompt, today's prefill_prompt call; ends on the sampled EOS: P + n rows
    got = gen.generate_codes(*new1, 40, 0.9, 50, session=conv)
    assert torch.equal(got[:, 0], frames[:11].to(torch.int32))
    assert model.log[:2] == [("reset_caches",), ("prefill_prompt", 20, None)] and not [e for e in model.log if e[0] == "load"]
    assert model.log[-1] == ("save", 0, 0, 0, 20 + 11) and model.log[-2] == ("read",), "the save follows the last block's read"
    assert conv.rows == 31 and conv.turns == 1 and torch.equal(conv.replies[0], frames[:11].t().to(torch.int32))
    cold2 = _cat(new1, _audio_rows(frames[:11]), EOS_ROW, new2)
    # turn 2: load, then ONLY the rows the session does not hold; cut at its limit of 6 frames: P + n - 1 rows
    del model.log[:]
    got = gen.generate_codes(*new2, 6, 0.9, 50, session=conv)
    assert got.shape[0] == 6
    assert model.log[:3] == [("reset_caches",), ("load", [0], [0], [31]), ("prefill_prompt", 36, 31)]
    assert torch.equal(model.prompts[-1][0], cold2[0]) and torch.equal(model.prompts[-1][1], cold2[1]), "the full prompt is the cold call's"
    assert model.log[-1] == ("save", 0, 0, 31, 36 + 6 - 1) and model.log[-2] == ("read",)
    assert conv.rows == 41 and conv.tokens.shape[0] == 42, "the mirror holds all 6 frames, the pages all but the last one's row"
    # turn 3: the suffix starts with reply 2's last frame, then the EOS row, then the new rows
    cold3 = _cat(cold2, _audio_rows(frames[:6]), EOS_ROW, new3)
    del model.log[:]
    gen.generate_codes(*new3, 40, 0.9, 50, session=conv)
    assert model.log[:3] == [("reset_caches",), ("load", [0], [0], [41]), ("prefill_prompt", 46, 41)]
    assert torch.equal(model.prompts[-1][0], cold3[0]) and torch.equal(model.prompts[-1][1], cold3[1])
    suffix = model.prompts[-1][0][41:]
    assert torch.equal(suffix[0, :32], frames[5].long()) and not bool(suffix[1].any()) and torch.equal(suffix[2:], new3[0])
    assert model.log[-1] == ("save", 0, 0, 41, 46 + 11) and conv.turns == 3
    # a limit <= 0 generates nothing and leaves the session as it was; too long a history is the existing ValueError
    del model.log[:]
    assert gen.generate_codes(*new3, 0, 0.9, 50, session=conv).shape[0] == 0
    assert conv.turns == 3 and conv.rows == 57 and not [e for e in model.log if e[0] in ("save", "load")]
    with pytest.raises(ValueError, match="Inputs too long"):
        gen.generate_codes(*new3, 2048 - 61, 0.9, 50, session=conv)          # 57 + 1 + 3 rows
    # session=None: the model sees today's calls
    del model.log[:]
    gen.generate_codes(*new3, 6, 0.9, 50)
    assert model.log[:2] == [("reset_caches",), ("prefill_prompt", 3, None)] and not [e for e in model.log if e[0] in ("save", "load")]
    # generate / generate_stream take the session too: the turn's text rows are new rows
    gen.generate([8, 9], 0, [], max_audio_length_ms=4 * 80, session=conv)
    assert conv.turns == 4 and model.log[-1][:1] == ("save",)
    list(gen.generate_stream([8, 9, 10], 0, [], max_audio_length_ms=40 * 80, session=conv))
    assert conv.turns == 5 and conv.tokens.shape[0] == 57 + 1 + 2 + 4 + 1 + 3 + 11
    conv.close()
    with pytest.raises(ValueError):
        gen.generate_codes(*new3, 6, 0.9, 50, session=conv)


def test_truncate_last_cuts_mirror_and_pages():
    from sesameai.generator import Generator
    script = _scripted(64, 1, [11])
    frames = script[:, 0]
    model = _One(script)
    gen = Generator(model, audio_tokenizer=_FakeCodec())
    conv = gen.open_session()
    new1, new2 = _rows(list(range(100, 112))), _rows([1, 2, 3])
    with pytest.raises(ValueError):
        conv.truncate_last(0)                                   # no reply yet
    gen.generate_codes(*new1, 40, 0.9, 50, session=conv)        # 12 + 11 rows
    with pytest.raises(ValueError):
        conv.truncate_last(12)
    conv.truncate_last(4)                                       # the listener heard 4 frames
    assert ("truncate", 0, 16) in model.log and conv.rows == 16 and conv.tokens.shape[0] == 16 and conv.replies[0].shape == (32, 4)
    del model.log[:]
    gen.generate_codes(*new2, 5, 0.9, 50, session=conv)         # cut at its limit: 20 + 5 - 1 rows
    cold = _cat(new1, _audio_rows(frames[:4]), EOS_ROW, new2)
    assert model.log[1:3] == [("load", [0], [0], [16]), ("prefill_prompt", 20, 16)]
    assert torch.equal(model.prompts[-1][0], cold[0]) and torch.equal(model.prompts[-1][1], cold[1])
    assert conv.rows == 24
    del model.log[:]
    conv.truncate_last(5)                                       # all 5 frames were heard: the pages hold 4 of their rows already, nothing to cut
    assert not model.log and conv.rows == 24 and conv.tokens.shape[0] == 25
    conv.truncate_last(0)
    assert model.log == [("truncate", 0, 20)] and conv.rows == 20 and conv.tokens.shape[0] == 20


def _turn(gen, model, news, sessions, limit, **kw):
    """One call of the live batch; returns (full prompts, log, frames)."""
    full = [(t, mk) if c is None else c.full_prompt(t, mk) for (t, mk), c in zip(news, sessions)]
    held = [0 if c is None else c.rows for c in sessions]
    del model.log[:]
    out = gen.generate_codes_continuous(news, limit, 0.9, 50, sessions=sessions, **kw)
    return full, held, list(model.log), out


def _check_turn(model_cls, lens, limit, sessions, full, held, log, out, scripts, pids):
    for j, pid in enumerate(pids):
        assert torch.equal(out[j], scripts[pid][: min(lens[pid], limit)].to(torch.int32)), f"request {j}"
    by_pid = {pid: j for j, pid in enumerate(pids)}
    refill = {}                                                 # request -> (log index, slot)
    for k, e in enumerate(log):
        if e[0] in ("refill_slot", "refill_begin"):
            j = by_pid[e[2]]
            refill[j] = (k, e[1])
            S = full[j][0].shape[0]
            assert e[3] == S - held[j] and e[4] == ({"start": held[j]} if held[j] else {}), f"request {j}: only the rows its session lacks run"
            if held[j]:
                assert log[k - 1] == ("load", [sessions[j].device.sid], [e[1]], [held[j]]), f"request {j}: the load is the call right before the refill"
        if e[0] == "group_begin":
            js = [by_pid[p] for p in e[2]]
            for j, slot, rows, start in zip(js, e[1], e[3], e[4]):
                refill[j] = (k, slot)
                assert rows == full[j][0].shape[0] - held[j] and start == held[j]
            warm = [(sessions[j].device.sid, slot, held[j]) for j, slot in zip(js, e[1]) if held[j]]
            if warm:
                assert log[k - 1] == ("load", [w[0] for w in warm], [w[1] for w in warm], [w[2] for w in warm]), "ONE load for the group, right before its begin"
            else:
                assert log[k - 1][0] != "load"
    assert sorted(refill) == list(range(len(pids)))
    assert len([e for e in log if e[0] == "load"]) == len({refill[j][0] for j in refill if held[j]}), "no load without its refill"
    for j, c in enumerate(sessions):
        saves = [(k, e) for k, e in enumerate(log) if e[0] == "save" and c is not None and e[1] == c.device.sid]
        if c is None:
            continue
        (ks, e), = saves
        P, n = full[j][0].shape[0], out[j].shape[0]
        assert e[2] == refill[j][1] and e[3] == held[j] and e[4] == (P + n if n < limit else P + n - 1), f"request {j}: {e}"
        kr = max(k for k in range(ks) if log[k][0] in ("read", "refill_slot"))        # (an empty reply of the stalling refill is known without a read)
        between = log[kr + 1:ks]
        assert not [x for x in between if x[0] == "step"], "a frame step between the read and the save"
        assert not [x for x in between if x[0] == "reset_slots" and e[2] in x[1]], "the slot was rewound before its rows were saved"
        assert not [x for x in between if x[0] in ("refill_slot", "refill_begin") and x[1] == e[2]], "the slot was refilled before its rows were saved"
        assert not [x for x in between if x[0] == "group_begin" and e[2] in x[1]]
        assert c.rows == e[4] and c.tokens.shape[0] == P + n


@pytest.mark.parametrize("model_cls, group", [(_SlotsS, 1), (_BesideS, 1), (_GroupS, 4)])
def test_live_batch_loads_before_the_refill_and_saves_before_the_slot_moves_on(model_cls, group):
    from sesameai.generator import Generator
    lens = [3, 9, 0, 5, 14, 2, 7, 12, 4, 12, 6, 1, 8, 0]        # scripts 0..6: turn 1, 7..13: turn 2; 12 = the length limit
    scripts = _scripts(lens, 21)
    model = model_cls(scripts, 3)
    gen = Generator(model, audio_tokenizer=_FakeCodec(), max_batch_size=3)
    gen.refill_row_layers = 40
    convs = [gen.open_session() for _ in range(5)]
    sessions = [convs[0], None, convs[1], convs[2], None, convs[3], convs[4]]       # two plain requests among five conversations
    kw = {"refill_group": group} if group > 1 else {}
    news1 = [_rows([300 + 10 * j + r for r in range(4 + j)] + [j]) for j in range(7)]
    full, held, log, out = _turn(gen, model, news1, sessions, 12, **kw)
    assert held == [0] * 7 and not [e for e in log if e[0] == "load"]
    _check_turn(model_cls, lens, 12, sessions, full, held, log, out, scripts, list(range(7)))
    assert all(c.turns == 1 for c in convs)
    # turn 2: every conversation is warm; the plain requests run whole, as without sessions
    news2 = [_rows([600 + j, 7 + j]) for j in range(7)]
    full, held, log, out = _turn(gen, model, news2, sessions, 12, **kw)
    assert [h > 0 for h in held] == [c is not None for c in sessions]
    for j, c in enumerate(sessions):
        if c is not None:
            n1 = min(lens[j], 12)
            want = _cat(news1[j], _audio_rows(scripts[j][:n1]), EOS_ROW, news2[j])
            assert torch.equal(full[j][0], want[0]) and torch.equal(full[j][1], want[1]), "the full prompt of turn 2 is the cold call's"
            assert held[j] == news1[j][0].shape[0] + (n1 if n1 < 12 else n1 - 1)
    _check_turn(model_cls, lens, 12, sessions, full, held, log, out, scripts, list(range(7, 14)))
    assert all(c.turns == 2 for c in convs)
    if group > 1:
        assert max(len(e[1]) for e in log if e[0] == "load") >= 2, "several sessions of one group share one load"
    # sessions=None / no Conversation in the list: neither call reaches the model
    del model.log[:]
    gen.generate_codes_continuous(news1, 12, 0.9, 50, sessions=[None] * 7, **kw)
    assert not [e for e in model.log if e[0] in ("load", "save")]


def test_one_request_per_session_and_one_entry_per_request():
    from sesameai.generator import Generator
    scripts = _scripts([3, 3, 3], 5)
    model = _BesideS(scripts, 3)
    gen = Generator(model, audio_tokenizer=_FakeCodec(), max_batch_size=3)
    a, b = gen.open_session(), gen.open_session()
    news = [_rows([50, j]) for j in range(3)]
    del model.log[:]
    with pytest.raises(ValueError, match="one request per session"):
        gen.generate_codes_continuous(news, 12, 0.9, 50, sessions=[a, b, a])
    with pytest.raises(ValueError):
        gen.generate_codes_continuous(news, 12, 0.9, 50, sessions=[a, b])
    with pytest.raises(ValueError):
        gen.generate_codes(torch.stack([news[0][0], news[1][0]]), torch.stack([news[0][1], news[1][1]]), 12, 0.9, 50, session=a)
    assert model.log == [] and a.turns == 0 and a.tokens.shape[0] == 0


@pytest.mark.parametrize("model_cls", [_SlotsS, _BesideS])
def test_a_short_pool_evicts_the_least_recently_used_session_which_then_runs_cold(model_cls):
    from sesameai.generator import Generator
    lens = [5, 6, 4, 3, 2, 7]
    scripts = _scripts(lens, 8)
    model = model_cls(scripts, 2)
    model.pool_pages = 6                                        # 48 rows
    gen = Generator(model, audio_tokenizer=_FakeCodec(), max_batch_size=2)
    a, b, c = gen.open_session(), gen.open_session(), gen.open_session()
    # a (17 + 5 rows: 3 pages) and b (10 + 6 rows: 2 pages) take 5 of the 6 pages, one call each
    gen.generate_codes_continuous([_rows(list(range(100, 116)) + [0])], 12, 0.9, 50, sessions=[a])
    gen.generate_codes_continuous([_rows(list(range(200, 209)) + [1])], 12, 0.9, 50, sessions=[b])
    assert (a.rows, b.rows) == (22, 16) and a.evictions == b.evictions == 0
    # c's first turn (8 + 4 rows: 2 pages) needs pages: a, used longest ago, loses its pages and keeps its mirror
    del model.log[:]
    gen.generate_codes_continuous([_rows(list(range(400, 407)) + [2])], 12, 0.9, 50, sessions=[c])
    k = next(k for k, e in enumerate(model.log) if e[0] == "save_refused")
    assert model.log[k:k + 3] == [("save_refused", 2), ("truncate", 0, 0), ("save", 2, model.log[k + 2][2], 0, 12)]
    assert (a.rows, b.rows, c.rows) == (0, 16, 12) and a.evictions == 1 and a.tokens.shape[0] == 22 and a.turns == 1
    # a's next turn runs cold from the full mirror -- no load, the whole prompt, no `start` -- and its save (29 rows: 4 pages) evicts b (c was used later)
    del model.log[:]
    new = _rows([1, 2, 3])
    full = a.full_prompt(*new)
    assert full[0].shape[0] == 22 + 1 + 3
    out = gen.generate_codes_continuous([new], 12, 0.9, 50, sessions=[a])
    assert torch.equal(out[0], scripts[3][:3].to(torch.int32))
    e = next(e for e in model.log if e[0] in ("refill_slot", "refill_begin"))
    assert e[3] == 26 and e[4] == {} and not [x for x in model.log if x[0] == "load"]
    assert ("truncate", 1, 0) in model.log and (a.rows, b.rows, c.rows) == (29, 0, 12) and b.evictions == 1
    # two sessions in ONE call that do not fit together: the running call's are never evicted, the one that saves second goes cold itself
    del model.log[:]
    out = gen.generate_codes_continuous([_rows([4]), _rows(list(range(60, 68)) + [5])], 12, 0.9, 50, sessions=[b, c])
    assert torch.equal(out[0], scripts[4][:2].to(torch.int32)) and torch.equal(out[1], scripts[5][:7].to(torch.int32)), "no request fails for lack of pages"
    assert a.rows == 0 and a.evictions == 2, "a was outside the call: b's save (18 + 2 rows: 3 pages) evicted it"
    assert b.rows == 20 and b.evictions == 1
    assert c.rows == 0 and c.evictions == 1, "c (22 + 7 rows: 4 pages beside b's 3) could evict nobody: it went cold itself"
    assert not [e for e in model.log if e[0] == "truncate" and e[1] == 1], "a session of the running call is never evicted by another's save"
    assert b.turns == 2 and c.turns == 2 and b.tokens.shape[0] == 20 and c.tokens.shape[0] == 29
