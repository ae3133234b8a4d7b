"""The session store on the GPU (include/csm_hip.h csm_session_*; Model.open_session_store / save_session / load_sessions): a conversation's
backbone K/V kept in fixed-size pages and copied, never recomputed.

The copy kernels move bits, so every comparison is ``torch.equal`` with no excused rows: a session's ``read()`` against the prefix store's
``capture_prefix(slot, rows).read()`` of the slot it was saved from (both dense, one layout), and a loaded slot's capture against the
source's.  What the copies must NOT touch is checked the same way: a slot that no load lists, and a target slot's rows at and beyond the
session's row count."""
import ctypes
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAGE = 8          # rows per page of the tiny store: 23 rows = two full pages and 7 rows of a third
ROWS = 40         # rows every tiny slot holds


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _cap(m, slot, rows):
    p = m.capture_prefix(slot, rows)
    out = p.read()
    p.destroy()
    return out


def _slot_prompt(slot):
    from oracle import csm_ref as C
    from oracle.make_golden import toy_prompt
    tok, msk = toy_prompt(C.csm_tiny(), 40 + slot, 10, ROWS)   # three different prompts: no two slots hold the same rows
    return tok[:ROWS], msk[:ROWS]


def _restore(m, slots):
    """The listed slots run their own prompts again (prompt mode: the same bits as the first time)."""
    for slot in slots:
        m.refill_slot(slot, *_slot_prompt(slot), 1.0, 1)


def _tiny_model(slots=3):
    from sesameai.models import Model, csm_tiny_2k_args, synthetic_state_dict
    m = Model(csm_tiny_2k_args(), synthetic_state_dict(csm_tiny_2k_args(), seed=1234), max_frames=16, max_prefill_rows=128)
    m.setup_caches(slots)
    m.reset_caches()
    _restore(m, range(slots))
    return m


@pytest.fixture(scope="module")
def tiny():
    """(a 3-slot tiny handle whose slots hold 40 rows each, the rows of each slot [L][2][KV][40][hd])."""
    _need_gpu()
    m = _tiny_model()
    want = [_cap(m, s, ROWS) for s in range(3)]
    assert not torch.equal(want[0], want[1]) and not torch.equal(want[1], want[2])
    assert all(bool((w.float().abs().sum(dim=(0, 1, 2, 4)) > 0).all()) for w in want), "a slot's row is all zero"
    m.open_session_store(12, PAGE)
    return m, want


def _slots_unchanged(m, want, slots=(0, 1, 2)):
    for s in slots:
        assert torch.equal(_cap(m, s, ROWS), want[s]), f"slot {s} changed"


def test_incremental_saves_equal_the_slots_rows(tiny):
    m, want = tiny
    s = m.open_session()
    assert s.rows == 0 and s.pages == 0 and s.read().shape[3] == 0
    for rows in (1, 7, 8, 9, 16, 23):                          # inside the first page, its last row, a page boundary, one past it, ...
        m.save_session(s, 0, rows)
        assert s.rows == rows and s.pages == (rows + PAGE - 1) // PAGE
        got = s.read()
        assert torch.equal(got, _cap(m, 0, rows)) and torch.equal(got, want[0][:, :, :, :rows]), f"after the save to {rows} rows"
    m.save_session(s, 0, 23)                                   # nothing new: accepted, nothing happens
    assert s.rows == 23 and "session_store=1 sessions, 3/12 pages" in m.describe()
    s.close()
    assert "session_store=0 sessions, 0/12 pages" in m.describe() and not s.alive
    _slots_unchanged(m, want)


def test_two_sessions_of_different_lengths_load_in_one_launch(tiny):
    m, want = tiny
    a, b = m.open_session(), m.open_session()
    m.save_session(a, 0, 23)
    m.save_session(b, 1, 9)
    m.load_sessions([a, b], [1, 2])                            # slot 1 <- slot 0's 23 rows, slot 2 <- slot 1's 9 rows; slot 0 is not listed
    got1, got2 = _cap(m, 1, ROWS), _cap(m, 2, ROWS)
    assert torch.equal(got1[:, :, :, :23], want[0][:, :, :, :23]) and torch.equal(got2[:, :, :, :9], want[1][:, :, :, :9])
    assert torch.equal(got1[:, :, :, 23:], want[1][:, :, :, 23:]), "the load wrote slot 1 at or beyond the session's 23 rows"
    assert torch.equal(got2[:, :, :, 9:], want[2][:, :, :, 9:]), "the load wrote slot 2 at or beyond the session's 9 rows"
    _slots_unchanged(m, want, [0])
    m.load_sessions([], [])                                    # an empty load is accepted
    a.close(); b.close()
    _restore(m, [1, 2])
    _slots_unchanged(m, want)


def test_pages_handed_out_in_scrambled_order(tiny):
    m, want = tiny
    s1, s2 = m.open_session(), m.open_session()
    m.save_session(s1, 0, 9)                                   # pages for s1, then s2, then s1 again: no session's pages are contiguous
    m.save_session(s2, 1, 17)
    m.save_session(s1, 0, 20)
    s1.close()                                                 # its pages go back in another order than they were handed out
    s3 = m.open_session()
    m.save_session(s3, 2, 20)                                  # ... and come out again for s3
    m.save_session(s2, 1, 30)
    s4 = m.open_session()
    m.save_session(s4, 0, 23)
    assert torch.equal(s2.read(), want[1][:, :, :, :30]) and torch.equal(s3.read(), want[2][:, :, :, :20]) and torch.equal(s4.read(), want[0][:, :, :, :23])
    assert "session_store=3 sessions, 10/12 pages" in m.describe()
    m.load_sessions([s2, s3, s4], [1, 2, 0])                   # every slot gets its own rows back: nothing may change
    _slots_unchanged(m, want)
    for s in (s2, s3, s4):
        s.close()


def test_truncate_mid_page_then_append(tiny):
    m, want = tiny
    s = m.open_session()
    m.save_session(s, 0, 23)
    s.truncate(11)                                             # the second page stays (3 rows of it), the third goes back
    assert s.rows == 11 and s.pages == 2 and torch.equal(s.read(), want[0][:, :, :, :11])
    m.save_session(s, 1, 20)                                   # appends rows [11, 20) -- of slot 1
    assert s.pages == 3 and torch.equal(s.read(), torch.cat([want[0][:, :, :, :11], want[1][:, :, :, 11:20]], dim=3))
    s.truncate(0)
    assert s.rows == 0 and s.pages == 0
    m.save_session(s, 2, 8)
    assert torch.equal(s.read(), want[2][:, :, :, :8])
    s.close()


def test_refusals_leave_the_session_unchanged(tiny):
    from sesameai._abi import CsmError, lib
    from sesameai.models import SessionPoolFull
    m, want = tiny
    s = m.open_session()
    m.save_session(s, 0, 17)
    before = s.read()
    stream = torch.cuda.current_stream().cuda_stream

    def refused(code, call):
        with pytest.raises(CsmError) as e:
            call()
        assert e.value.code == code, str(e.value)
        assert s.rows == 17 and s.pages == 3 and torch.equal(s.read(), before)

    refused(-3, lambda: m.open_session_store(4, PAGE))         # one store per handle
    refused(-1, lambda: m.save_session(s, 0, 16))              # below the session's row count
    refused(-1, lambda: m.save_session(s, 0, m.bb.max_seq_len))
    refused(-1, lambda: m.save_session(s, 3, 20))              # a slot outside the batch
    refused(-1, lambda: m.load_sessions([s], [3]))
    refused(-1, lambda: m.load_sessions([s], [-1]))
    refused(-1, lambda: m.load_sessions([s, s], [1, 1]))       # a slot listed twice
    refused(-1, lambda: s.truncate(18))
    # a session of another handle, and a closed one (the C call gets the stale pointer: the Python object refuses by itself)
    other = _tiny_model(1)
    other.open_session_store(2, PAGE)
    foreign = other.open_session()
    other.save_session(foreign, 0, 8)
    refused(-1, lambda: m.load_sessions([foreign], [1]))
    refused(-1, lambda: m.save_session(foreign, 0, 12))
    assert foreign.rows == 8
    gone = m.open_session()
    stale = gone._ptr().value
    gone.close()
    assert lib.csm_session_save(m._h, ctypes.c_void_p(stale), 0, 4, stream) == -1
    assert lib.csm_session_load(m._h, (ctypes.c_void_p * 1)(stale), (ctypes.c_int32 * 1)(1), 1, stream) == -1
    with pytest.raises(ValueError):
        m.save_session(gone, 0, 4)
    # a slot whose refill beside the loop is running
    assert m.supports_refill_beside_the_loop()
    m.refill_begin(2, *_slot_prompt(2))
    refused(-3, lambda: m.save_session(s, 2, 20))
    refused(-3, lambda: m.load_sessions([s], [2]))
    while not m.refill_advance(m.bb.num_layers):
        pass
    # a pool too short: 12 pages, 3 held by s, 5 by `big`: a second 40-row session needs 5 of the 4 left
    big, late = m.open_session(), m.open_session()
    m.save_session(big, 0, ROWS)
    with pytest.raises(SessionPoolFull):
        m.save_session(late, 1, ROWS)
    assert late.rows == 0 and late.pages == 0 and "session_store=3 sessions, 8/12 pages" in m.describe()
    m.save_session(late, 1, 32)                                # 4 pages: exactly what is left
    assert late.pages == 4 and torch.equal(late.read(), want[1][:, :, :, :32]) and torch.equal(big.read(), want[0])
    with pytest.raises(SessionPoolFull):
        m.save_session(s, 0, 25)
    assert s.rows == 17 and s.pages == 3 and torch.equal(s.read(), before)
    big.truncate(30)                                           # the host evicts a page and retries
    m.save_session(s, 0, 25)
    assert torch.equal(s.read(), want[0][:, :, :, :25]) and torch.equal(big.read(), want[0][:, :, :, :30])
    for x in (big, late, s, foreign):
        x.close()
    _slots_unchanged(m, want, [0, 1])


def test_csm1b_shapes_with_64_row_pages():
    """CSM-1B cache geometry (16 layers, 8 kv heads, head_dim 64: 256 runs, 8 KB per run and page) and a 1,334-row slot: 21 pages."""
    _need_gpu()
    import bench
    from types import SimpleNamespace
    from sesameai.models import Model, csm_1b_args
    a = SimpleNamespace(ctx_text=40, ctx_frames=125, gen_text=24)
    m = Model(csm_1b_args(), None, max_frames=8, max_prefill_rows=2048)
    m.setup_caches(2)
    m.reset_caches()
    S = 1334
    for slot in (0, 1):
        t, mk = bench.synthetic_prompt(a, 1, 128_256, seed0=5000 + slot, segments=10, ctx_text=30, ctx_frames=100)
        assert t.shape[1] == S
        m.refill_slot(slot, t[0], mk[0], 1.0, 1)
    want0, want1 = _cap(m, 0, S), _cap(m, 1, S)
    assert not torch.equal(want0, want1)
    m.open_session_store(24, 64)
    s = m.open_session()
    m.save_session(s, 0, 700)
    assert s.pages == 11 and torch.equal(s.read(), want0[:, :, :, :700])
    m.load_sessions([s], [1])
    got = _cap(m, 1, S)
    assert torch.equal(got[:, :, :, :700], want0[:, :, :, :700]) and torch.equal(got[:, :, :, 700:], want1[:, :, :, 700:])
    m.save_session(s, 0, S)
    assert s.pages == 21 and torch.equal(s.read(), want0) and "session_store=1 sessions, 21/24 pages" in m.describe()
    m.load_sessions([s], [1])
    assert torch.equal(_cap(m, 1, S), want0) and torch.equal(_cap(m, 0, S), want0)
    s.close()


# ----------------------------------------------------------------------------------------
# three-turn conversations, greedy, against the ORACLE's cold codes (oracle/csm_ref.py, run here on the CPU)
# ----------------------------------------------------------------------------------------
# The checkpoint is the history-dependent decisive one (oracle.csm_ref.decisive_copy_weights) with a lag of 20 rows: c0 of frame f names the
# last code of the row 20 back, read out of the copy layer's cached K / V.  A turn's suffix (the last frame's row, the EOS row, the user's
# segment, the reply's text) is 14 rows, so the first six frames of turns 2 and 3 are decided by LOADED rows -- rows that decode steps wrote
# a turn ago and that went through a save and a load -- and every margin is >= 4 x the bf16 gap between the two ways of writing a row.
# Sampled runs are not comparable (the prefix store's tests say why), so everything is greedy (top-k 1).
LAG = 20
FLAVOUR = f"decisive_copy:1:{LAG}"
N = 8             # frames per reply: every reply is cut at its limit (the copy trajectory never samples EOS)


def _generator(model, codec=None, batch=1):
    from sesameai.generator import Generator
    gen = Generator.__new__(Generator)
    gen._model, gen.device, gen._eos_poll, gen._audio_tokenizer, gen._text_tokenizer = model, model.device, 8, codec, None
    gen._max_batch, gen._stream_buffer_size, gen._mimi_stream, gen.sample_rate = batch, 10, None, 24_000
    return gen


def _dialogue(shape, c, turns=3):
    """Conversation c: per turn (the NEW segments [(text ids, codes (32, T))], the reply's text ids).  Turn 1 brings the voice prompt."""
    g = torch.Generator().manual_seed(500 + c)
    ids = lambda k: torch.randint(0, shape.text_vocab_size, (k,), generator=g).tolist()
    codes = lambda k: torch.randint(0, 2048, (shape.audio_num_codebooks, k), generator=g)
    out = [([(ids(5), codes(20 + c))], ids(4))]
    for _ in range(turns - 1):
        out.append(([(ids(3), codes(4))], ids(4)))
    return out


_ORACLE = {}


def _oracle_dialogues(dtype, keep=None):
    """Per conversation c and turn k: dict(new=(tokens, mask) of the NEW rows, full=the cold prompt, codes=the oracle's cold greedy codes
    (N, 32)).  ``keep``: {(c, k): frames of reply k the listener heard} -- the cold context of the later turns holds only those (then only
    conversation 0's first two turns are run).  Computed once per (dtype, keep) and shared."""
    key = (dtype, tuple(sorted((keep or {}).items())))
    if key in _ORACLE:
        return _ORACLE[key]
    from oracle import csm_ref as C
    shape = C.csm_tiny()
    w = C.make_weights(shape, seed=1234, flavour=FLAVOUR)
    om = C.OracleModel(shape, C.fp8_dequantized(w) if dtype == "fp8" else w)
    om.setup_caches(1)
    out = []
    for c in range(1 if keep else 3):
        segs, turns = [], []
        for k, (new, text) in enumerate(_dialogue(shape, c, 2 if keep else 3)):
            segs = segs + new
            full = C.build_prompt(segs + [(text, None)])
            fr = C.generate_codes(om, full[0], full[1], N * 80, 1.0, 1, greedy=True, max_seq_len=shape.backbone.max_seq_len)
            codes = torch.cat(fr).to(torch.int32)
            assert codes.shape[0] == N and torch.equal(codes, C.decisive_copy_expected_codes(shape, 1234, full[0], full[1], N, LAG)), "the oracle left the copy trajectory"
            turns.append(dict(new=C.build_prompt(new + [(text, None)]), full=full, codes=codes))
            heard = (keep or {}).get((c, k), N)
            segs = segs + [(text, codes[:heard].t().contiguous())]
        out.append(turns)
    _ORACLE[key] = out
    return out


def _tiny_copy_model(batch, dtype, pages=48):
    from sesameai.models import Model, csm_tiny_args, synthetic_state_dict
    m = Model(csm_tiny_args(), synthetic_state_dict(csm_tiny_args(), seed=1234, flavour=FLAVOUR), max_frames=64, max_prefill_rows=256, weights_dtype=dtype)
    m.setup_caches(batch)
    m.open_session_store(pages, PAGE)
    return m


def _loaded_rows_decide(full_rows, held):
    """Frame 0 of the turn reads row S - 1 - LAG: one of the rows the session's pages gave the slot."""
    return full_rows - 1 - LAG < held


@pytest.mark.parametrize("dtype", ["bf16", "fp8"])
def test_tiny_three_turns_at_batch_1_equal_the_oracles_cold_codes(dtype):
    _need_gpu()
    want = _oracle_dialogues(dtype)
    m = _tiny_copy_model(1, dtype)
    gen = _generator(m)
    convs = [gen.open_session() for _ in range(3)]
    for k in range(3):                                         # the conversations take turns: each finds slot 0 full of another's rows
        for c, conv in enumerate(convs):
            t = want[c][k]
            held, S = conv.rows, t["full"][0].shape[0]
            got = gen.generate_codes(*t["new"], N, 1.0, 1, session=conv)[:, 0]
            assert m.last_prefill_rows == S - held, f"conversation {c} turn {k}: {m.last_prefill_rows} rows ran, the suffix has {S - held}"
            assert torch.equal(got, t["codes"]), f"conversation {c} turn {k} differs from the oracle's cold codes"
            assert conv.rows == S + N - 1 and conv.turns == k + 1 and torch.equal(conv.tokens[:S], t["full"][0])
            if k:
                assert held == want[c][k - 1]["full"][0].shape[0] + N - 1 and _loaded_rows_decide(S, held)
    assert f"session_store=3 sessions, {sum(c.device.pages for c in convs)}/48 pages" in m.describe()
    # the same turn without a session is the cold call
    t = want[0][2]
    assert torch.equal(gen.generate_codes(*t["full"], N, 1.0, 1)[:, 0], t["codes"]) and m.last_prefill_rows == t["full"][0].shape[0]


def _live_turns(gen, m, want, convs, group, dtype):
    """Three calls of the live batch: request order (c0, plain, c1, c2, plain) through 4 slots, so one request is refilled inside the batch."""
    plain = want[0][0]["full"], want[1][0]["full"]             # two requests without a session: cold prompts of their own
    for k in range(3):
        reqs = [want[0][k]["new"], plain[0], want[1][k]["new"], want[2][k]["new"], plain[1]]
        sessions = [convs[0], None, convs[1], convs[2], None]
        held = [0 if c is None else c.rows for c in sessions]
        fulls = [want[0][k]["full"], plain[0], want[1][k]["full"], want[2][k]["full"], plain[1]]
        rows0 = m.prefill_rows_total
        got = gen.generate_codes_continuous(reqs, N, 1.0, 1, sessions=sessions, **group)
        ran = m.prefill_rows_total - rows0
        assert ran == sum(f[0].shape[0] - h for f, h in zip(fulls, held)), f"turn {k}: {ran} rows ran -- a silent cold fallback, or rows run twice"
        codes = [want[0][k]["codes"], want[0][0]["codes"], want[1][k]["codes"], want[2][k]["codes"], want[1][0]["codes"]]
        for i, (g, w) in enumerate(zip(got, codes)):
            assert torch.equal(g, w), f"turn {k} request {i} differs from the oracle's cold codes"
        if k:
            assert all(h > 0 and _loaded_rows_decide(f[0].shape[0], h) for f, h, c in zip(fulls, held, sessions) if c is not None)
        if k == 1:                                             # the same requests with no sessions at all: the plain requests' frames are the same
            cold = gen.generate_codes_continuous(fulls, N, 1.0, 1, **group)
            assert all(torch.equal(a, b) for a, b in zip(cold, got))


@pytest.mark.parametrize("beside", [True, False])
@pytest.mark.parametrize("dtype", ["bf16", "fp8"])
def test_tiny_three_turns_in_the_live_batch_through_both_refill_paths(dtype, beside):
    _need_gpu()
    want = _oracle_dialogues(dtype)
    m = _tiny_copy_model(4, dtype)
    gen = _generator(m, batch=4)
    gen.refill_beside_the_loop = beside
    gen.refill_row_layers = 40
    assert m.supports_refill_beside_the_loop(4)
    _live_turns(gen, m, want, [gen.open_session() for _ in range(3)], {}, dtype)


def test_tiny_three_sessions_and_a_plain_request_in_one_refill_group():
    _need_gpu()
    want = _oracle_dialogues("bf16")
    m = _tiny_copy_model(4, "bf16")
    gen = _generator(m, batch=4)
    gen.refill_row_layers = 40
    _live_turns(gen, m, want, [gen.open_session() for _ in range(3)], {"refill_group": 4}, "bf16")


def test_tiny_truncate_last_equals_the_cold_run_with_the_frames_heard():
    """Barge-in: the listener heard 3 of reply 1's 8 frames.  Turn 2 equals the oracle's cold run whose context holds only those 3."""
    _need_gpu()
    want = _oracle_dialogues("bf16", keep={(0, 0): 3})
    m = _tiny_copy_model(1, "bf16")
    gen = _generator(m)
    conv = gen.open_session()
    t1, t2 = want[0][0], want[0][1]
    assert torch.equal(gen.generate_codes(*t1["new"], N, 1.0, 1, session=conv)[:, 0], t1["codes"])
    P = t1["full"][0].shape[0]
    assert conv.rows == P + N - 1
    conv.truncate_last(3)
    assert conv.rows == P + 3 and conv.device.pages == (P + 3 + PAGE - 1) // PAGE
    S = t2["full"][0].shape[0]
    assert S == P + 3 + 1 + t2["new"][0].shape[0] and _loaded_rows_decide(S, P + 3)
    got = gen.generate_codes(*t2["new"], N, 1.0, 1, session=conv)[:, 0]
    assert m.last_prefill_rows == S - (P + 3) and torch.equal(conv.tokens[:S], t2["full"][0])
    assert torch.equal(got, t2["codes"]), "turn 2 after truncate_last(3) differs from the cold run that holds 3 frames of reply 1"
    assert not torch.equal(got, _oracle_dialogues("bf16")[0][1]["codes"]), "the frames cut away do not matter to turn 2: this case shows nothing"


def test_tiny_a_store_too_small_for_two_sessions_still_gives_the_oracles_codes():
    _need_gpu()
    want = _oracle_dialogues("bf16")
    m = _tiny_copy_model(1, "bf16", pages=12)                  # 96 rows: one conversation's third turn needs 10 pages, two need 16
    gen = _generator(m)
    convs = [gen.open_session() for _ in range(2)]
    cold_turns = 0
    for k in range(3):
        for c, conv in enumerate(convs):
            t = want[c][k]
            held, S = conv.rows, t["full"][0].shape[0]
            got = gen.generate_codes(*t["new"], N, 1.0, 1, session=conv)[:, 0]
            assert torch.equal(got, t["codes"]), f"conversation {c} turn {k}"
            assert m.last_prefill_rows == S - held
            cold_turns += int(k > 0 and held == 0)
            used = sum(x.device.pages for x in convs)
            assert used <= 12 and f"session_store=2 sessions, {used}/12 pages" in m.describe()
    assert cold_turns >= 1 and sum(c.evictions for c in convs) >= 1, "the pool was never short: this case shows nothing"
    assert all(c.turns == 3 and c.tokens.shape[0] == want[i][2]["full"][0].shape[0] + N for i, c in enumerate(convs))


def test_tiny_generate_many_stream_with_sessions_yields_each_requests_whole_clip():
    _need_gpu()
    from sesameai.generator import Segment
    from sesameai.mimi import MimiArgs, MimiCodec, synthetic_state_dict as mimi_sd
    from oracle import csm_ref as C
    want = _oracle_dialogues("bf16")
    m = _tiny_copy_model(3, "bf16")
    codec = MimiCodec(MimiArgs(), mimi_sd(MimiArgs(), seed=4321), max_frames=96)
    gen = _generator(m, codec, batch=3)
    convs = [gen.open_session(), gen.open_session()]
    shape = C.csm_tiny()
    for k in range(2):
        texts, contexts = [], []
        for c in range(3):                                     # requests 0 and 1 are turns of conversations, request 2 is plain and brings its whole history
            turns = _dialogue(shape, c)
            new, text = turns[k]
            segs = list(new)
            if c == 2:                                         # the cold context: every earlier turn's new segments and its reply, then this turn's
                segs = [x for kk in range(k) for x in turns[kk][0] + [(turns[kk][1], want[c][kk]["codes"].t())]] + segs
            texts.append(text)
            contexts.append([Segment(speaker=0, text=ids, audio_codes=codes) for ids, codes in segs])
        pcm, frames = {}, {}
        for i, chunk, fr, last in gen.generate_many_stream(texts, [0] * 3, contexts, max_audio_length_ms=N * 80, temperature=1.0, topk=1,
                                                           sessions=[convs[0], convs[1], None]):
            pcm.setdefault(i, []).append(chunk.cpu()); frames.setdefault(i, []).append(fr)
        for i in range(3):
            fr = torch.cat(frames[i])
            assert torch.equal(fr, want[i][k]["codes"]), f"turn {k} request {i}: codes"
            whole = gen._decode_frames(fr.unsqueeze(1)).cpu()
            assert torch.equal(torch.cat(pcm[i]), whole), f"turn {k} request {i}: the chunks, concatenated, are not the whole-clip decode"


# ----------------------------------------------------------------------------------------
# CSM-1B shapes: tests/golden/csm1b_sessions.pt (tools/make_session_golden.py) -- the s1334 copy checkpoint (copy layer 3, lag 700)
# ----------------------------------------------------------------------------------------
# Turn 1 is the 1,334-row prompt of csm1b_decisive_copy.pt; turns 2 and 3 add 23 new rows each.  c0 of a frame names the last code of the
# row 700 back: turn 2's and turn 3's decisions are all read through rows that a session's pages carried (the golden holds the oracle-only
# proof that zeroing those rows, or moving their values one position, changes the codes).
_S1B = {}


def _s1334():
    import bench
    from types import SimpleNamespace
    a = SimpleNamespace(ctx_text=40, ctx_frames=125, gen_text=24)
    t, m = bench.synthetic_prompt(a, 1, 128_256, seed0=5000, segments=10, ctx_text=30, ctx_frames=100)
    return t[0], m[0]


@pytest.fixture(scope="module")
def sessions1b():
    """(gold, turns(dtype) -> per turn dict(new, full, codes, held), get(dtype) -> an 8-slot CSM-1B handle with a 176-page session store)."""
    _need_gpu()
    from sesameai.models import Model, csm_1b_args, synthetic_state_dict
    gold = torch.load(os.path.join(ROOT, "tests", "golden", "csm1b_sessions.pt"))
    assert all(min(t["faults_changed"].values()) > 0 for tag in ("bf16", "fp8") for t in gold[tag][1:]), "the golden cannot see a fault in the carried rows"
    sd = synthetic_state_dict(csm_1b_args(), seed=int(gold["weight_seed"]), flavour=gold["flavour"])
    names, sums = gold["weight_checksums"]
    assert torch.equal(torch.stack([sd[k].view(torch.int16).to(torch.int64).sum() for k in names]), sums), "not the checkpoint the oracle's codes were generated with"
    first = _s1334()
    assert first[0].shape[0] == int(gold["prompt_rows"]) == 1334

    def turns(dtype):
        out, hist = [], None
        for k, t in enumerate(gold[dtype]):
            new = first if k == 0 else (t["new_tokens"].long(), t["new_mask"])
            full = new if k == 0 else tuple(torch.cat([h, e, x]) for h, e, x in zip(hist, _EOS_ROW, new))
            codes = t["codes"].to(torch.int32)
            assert full[0].shape[0] == int(t["full_rows"])
            out.append(dict(new=new, full=full, codes=codes, held=int(t["held"])))
            ft = torch.zeros(codes.shape[0], 33, dtype=torch.long); ft[:, :32] = codes.long()
            fm = torch.zeros(codes.shape[0], 33, dtype=torch.bool); fm[:, :32] = True
            hist = (torch.cat([full[0], ft]), torch.cat([full[1], fm]))
        return out

    def get(dtype):
        if dtype not in _S1B:
            _S1B.clear()                                       # one handle at a time
            m = Model(csm_1b_args(), sd, max_frames=96, max_prefill_rows=2048, weights_dtype=dtype)
            m.setup_caches(8)
            m.open_session_store(176, 64)
            _S1B[dtype] = m
        return _S1B[dtype]
    yield gold, turns, get
    _S1B.clear()


_EOS_ROW = (torch.zeros(1, 33, dtype=torch.long), torch.tensor([[True] * 32 + [False]]))


@pytest.mark.parametrize("dtype", ["bf16", "fp8"])
def test_csm1b_three_turns_at_batch_1_equal_the_golden(sessions1b, dtype):
    """generate_codes at B = 1: the one-launch backbone layer, the first decoder step's launch and the persistent decoder read the loaded rows."""
    gold, turns, get = sessions1b
    m, want = get(dtype), turns(dtype)
    n = int(gold["frames"])
    gen = _generator(m)
    conv = gen.open_session()
    for k, t in enumerate(want):
        held, S = conv.rows, t["full"][0].shape[0]
        assert held == t["held"]
        got = gen.generate_codes(*t["new"], n, 1.0, 1, session=conv)[:, 0]
        assert m.last_prefill_rows == S - held, f"turn {k}: {m.last_prefill_rows} rows ran, the suffix has {S - held}"
        assert torch.equal(got, t["codes"]), f"turn {k}: leaves the golden at frame {int((got != t['codes']).any(dim=1).nonzero()[0]) if got.shape == t['codes'].shape else got.shape}"
        assert conv.rows == S + n - 1 and conv.device.pages == (S + n - 1 + 63) // 64
    paths = m.fast_paths()
    assert paths & 1 and paths & 32 and paths & (16 if dtype == "fp8" else 8), f"an all-CU launch of the B = 1 step was off: {paths}"
    conv.close()
    assert "session_store=0 sessions, 0/176 pages" in m.describe()


def _live_1b(gen, m, want, n, group):
    """Nine requests through 8 slots, three turns: seven conversations of the golden's content and two plain requests with the turn's cold
    prompt (request 3: in the first refill group beside three sessions; request 8: refilled inside the batch)."""
    convs = [gen.open_session() for _ in range(7)]
    sessions = convs[:3] + [None] + convs[3:6] + [None] + convs[6:]
    assert len(sessions) == 9 and sessions[3] is None and sessions[7] is None
    for k, t in enumerate(want):
        S = t["full"][0].shape[0]
        held = [0 if c is None else c.rows for c in sessions]
        assert all(h == (t["held"] if c is not None else 0) for h, c in zip(held, sessions))
        reqs = [t["full"] if c is None else t["new"] for c in sessions]
        rows0 = m.prefill_rows_total
        got = gen.generate_codes_continuous(reqs, n, 1.0, 1, sessions=sessions, **group)
        assert m.prefill_rows_total - rows0 == sum(S - h for h in held), f"turn {k}: a silent cold fallback, or rows run twice"
        for i, g in enumerate(got):
            assert torch.equal(g, t["codes"]), f"turn {k} request {i} ({'plain' if sessions[i] is None else 'session'}) differs from the golden"
        if k == 1:                                             # no sessions at all: the plain requests' frames are the same
            cold = gen.generate_codes_continuous([t["full"]] * 9, n, 1.0, 1, **group)
            assert torch.equal(cold[3], got[3]) and torch.equal(cold[7], got[7])
    assert f"session_store=7 sessions, {7 * convs[0].device.pages}/176 pages" in m.describe()
    for c in convs:
        c.close()


@pytest.mark.parametrize("beside", [True, False])
@pytest.mark.parametrize("dtype", ["bf16", "fp8"])
def test_csm1b_three_turns_in_the_live_batch_of_8(sessions1b, dtype, beside):
    gold, turns, get = sessions1b
    m = get(dtype)
    gen = _generator(m, batch=8)
    gen.refill_beside_the_loop = beside
    _live_1b(gen, m, turns(dtype), int(gold["frames"]), {})


def test_csm1b_three_sessions_and_a_plain_request_in_one_refill_group(sessions1b):
    gold, turns, get = sessions1b
    m = get("fp8")                                             # (the handle the test before left)
    gen = _generator(m, batch=8)
    _live_1b(gen, m, turns("fp8"), int(gold["frames"]), {"refill_group": 4})
