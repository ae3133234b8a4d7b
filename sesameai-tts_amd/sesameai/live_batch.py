"""The continuously refilled batch behind ``Generator.iter_codes_continuous`` / ``generate_many`` / ``generate_many_stream``: ONE slot
scheduler (``LiveBatch``) with two ways of giving a free slot its next prompt (``_Stalling``, ``_BesideTheLoop``), and the consumer that
turns its polled blocks into streamed audio (``SlotStreams``).  Host code only; the reference (batch-1) has no counterpart."""
import contextlib
from collections import deque
from dataclasses import dataclass
from typing import Iterator, List, Optional, Sequence, Tuple

import torch

from .models import match_stored_prefix

_NO_FRAMES = torch.empty(0, 32, dtype=torch.int32)


@dataclass
class _Utterance:
    """What a batch slot holds while it generates."""
    index: int                          # of its prompt
    limit: int                          # frames
    first: int                          # global frame index of the first frame it takes from the history: its frame 0, or frame 1 when
    frames: List[torch.Tensor]          # the refill handed frame 0 over; the frames held so far
    reported: int = 0                   # how many of them were handed out


class LiveBatch:
    """A batch of ``slots`` slots kept full: every polled block's rows are cut per slot at the utterance's EOS or length limit and handed out
    as events ``(index of the prompt, batch slot, its NEW frames [k][32] int32 CPU, last)``, finished utterances are retired and their slots
    refilled while the others keep generating.  How a free slot gets its next prompt is the subclass's business -- ``_feed(everything)``: called
    after every queued frame step, and with ``everything`` when nobody generates (True: it did something); ``_vacated``, ``_idle``,
    ``_report_order`` -- the rest happens here, once.  The Philox key of a sampled frame includes the global frame index, so the number of
    frame steps between any two refill calls is part of the results (tests/test_live_batch_trace.py pins them) -- except for a prompt with a
    seed of its own (``own``), which draws at (its seed, its own frame index) wherever and whenever it runs.
    ``own[i]``: ``(temperature, topk, seed or None)`` of prompt ``i`` where it has values of its own, else None: the model's per-slot sampling
    table gets them (``Model.set_slot_sampling``) immediately before the prompt's refill call, and a slot such a prompt leaves is cleared
    before a prompt without own values takes it.  With no own values anywhere the model sees neither call.
    ``first_chunk`` = k (None: off, today's blocks exactly): while some utterance has had fewer than k of its frames handed out, a block of
    frame steps ends as soon as that utterance has k frames QUEUED -- evaluated after every queued step, because a refill may complete in the
    middle of a block -- so that its first audio need not wait for a whole block.  Otherwise blocks are ``poll`` steps as before.
    ``sessions[i]``: the ``Conversation`` (sesameai/sessions.py) prompt ``i`` is a turn of, or None; ``prompts[i]`` is then the session's FULL
    prompt.  The rows its pages hold are not run: the pages of all sessions of one refill call are loaded by ONE ``Model.load_sessions``
    immediately before that call (``_rows_to_run``), and when the turn is over its slot's new rows are saved -- after the block has been read,
    before the slot is rewound or refilled (``run``).  With no sessions (None) the model sees neither call.  An ``on_full="forget"`` session
    has dropped what its turn needs dropped BEFORE its full prompt was built (``sessions.make_room``, called by the Generator): its forget is
    on the stream ahead of every load of this batch, and ``warm`` below counts the rows its pages hold after it."""

    def __init__(self, model, prompts, limits: List[int], temperature: float, topk: int, poll: int, slots: int, store: list, own=None,
                 first_chunk: Optional[int] = None, sessions=None):
        self.m, self.prompts, self.limits, self.sampling, self.poll, self.B = model, prompts, limits, (temperature, topk), poll, slots
        self.first_chunk = first_chunk
        self.sessions = sessions if sessions is not None else [None] * len(prompts)
        # rows of prompt i that its session's pages hold (0: no session, or a cold one -- it runs like any prompt, through the prefix store);
        # fixed here: only a save can take a session's pages away, and never those of a session of the running call before its own turn is over
        self.warm = [min(c.rows, t.shape[0] - 1) if c is not None else 0 for c, (t, _) in zip(self.sessions, prompts)]
        self.own = own if own is not None else [None] * len(prompts)
        self.entries: set = set()                                   # slots that hold an entry of the sampling table (reset_caches empties it)
        # per prompt (rows P to copy, handle): the registered prefix with the longest match, (0, None) without one -- all matched before the loop
        # starts: no comparison's host synchronisation falls between frame steps; and {slot: handle} of the initial fill's shared copies
        self.plan = [match_stored_prefix(store, t, mk) for t, mk in prompts] if store else [(0, None)] * len(prompts)
        if sessions is not None:
            self.plan = [(0, None) if w else p for w, p in zip(self.warm, self.plan)]
        self.seeded = {slot: handle for slot, (_, handle) in enumerate(self.plan[:slots]) if handle is not None}
        self.pending = deque(range(len(prompts)))
        self.free = deque(range(slots))                             # slots waiting for a prompt
        self.slots: List[Optional[_Utterance]] = [None] * slots
        self.events: list = []                                      # of the current block
        self.g = 0                                                  # next global frame index to read

    def run(self) -> Iterator[Optional[list]]:
        """Per polled block a list of events; ``None`` each time a block's frame steps have just been queued (Generator._iter_blocks_continuous)."""
        m, B = self.m, self.B
        m.reset_caches()
        for handle in {id(h): h for h in self.seeded.values()}.values():    # all slots that start from the same prefix: ONE copy
            m.apply_prefix(handle, [slot for slot, h in self.seeded.items() if h is handle])
        self._feed(True)                                            # the initial fill: nothing to protect yet
        self.seeded.clear()
        self.g = m.num_frames()
        while True:
            if self.events:
                yield self.events
                self.events = []
            active = [u for u in self.slots if u is not None]
            if not active:
                if not self._feed(True):                            # only prompts left: finish them at full speed
                    return
                continue
            cuts = [(s, True) for s, u in enumerate(self.slots) if u is not None and u.frames and len(u.frames) >= u.limit]
            if not cuts:                                            # (else an utterance that came with its frame 0 is complete already: no steps)
                n = max(min(self.poll, min(u.limit - len(u.frames) for u in active)), 1)
                for done in range(1, n + 1):
                    m.step(B, *self.sampling)
                    self._feed(False)
                    if self.first_chunk is not None and self._first_chunk_queued(done):
                        n = done                                    # a short block: somebody's first chunk is ready to be read
                        break
                yield None                                          # (the block's steps are queued)
                cuts = self._read(n)
            for s, last in self._report_order(cuts):
                u = self.slots[s]
                fs = u.frames[u.reported:max(u.limit, 0)]           # the event: what is new, up to the limit
                u.reported += len(fs)
                if fs or last:
                    self.events.append((u.index, s, torch.stack(fs).to(torch.int32) if fs else _NO_FRAMES, last))
                if last:
                    self._turn_over(u.index, s, u.frames[:max(u.limit, 0)])
                    self.slots[s] = None
                    self._vacated(s)
            idle = self._idle([s for s, last in cuts if last])
            if idle and (self.pending or any(u is not None for u in self.slots)):
                m.reset_slots(idle)                                 # a retired slot keeps stepping: keep its position away from max_seq

    def _turn_over(self, i: int, slot: int, frames: List[torch.Tensor]) -> None:
        """Prompt ``i``'s utterance is over in ``slot`` with all ``frames`` handed out.  A session's turn: its slot's new rows go to its pages now
        (the block has been read; the slot has been neither rewound nor refilled).  A limit <= 0 generated nothing: the session stays as it was."""
        c = self.sessions[i]
        if c is not None and self.limits[i] > 0:
            t, mk = self.prompts[i]
            c.turn_over(self.m, slot, t, mk, torch.stack(frames) if frames else _NO_FRAMES, self.limits[i], [x for x in self.sessions if x is not None])

    def _first_chunk_queued(self, steps: int) -> bool:
        """Whether, ``steps`` queued steps into the block, an utterance that has had fewer than ``first_chunk`` frames handed out has that many
        queued (held, or sampled by this block's steps since it took its slot) -- or all its limit allows."""
        k = self.first_chunk
        for u in self.slots:
            if u is not None and u.reported < k:
                queued = len(u.frames) + max(0, self.g + steps - max(u.first, self.g))
                if queued >= min(k, u.limit):
                    return True
        return False

    def _read(self, n: int) -> List[Tuple[int, bool]]:
        """Reads the block of ``n`` steps and gives every slot its rows, cut at its EOS.  Returns [(slot, whether its utterance is over)]."""
        fr, eos = self.m.read_frames(self.B, self.g, n)            # waits for the block
        cuts = []
        for s, u in enumerate(self.slots):                          # (a slot may have joined during this block)
            lo = max(u.first - self.g, 0) if u is not None else n   # rows of this block that belong to the slot's current utterance
            if lo >= n:
                continue                                            # (nobody there, or it joined after this block's last step)
            rows, e = fr[lo:, s], int(eos[s])
            ended = e >= u.first
            if ended:
                rows = rows[: max(e - (self.g + lo), 0)]
            u.frames.extend(rows.unbind(0))
            cuts.append((s, ended or len(u.frames) >= u.limit))
        self.g += n
        return cuts

    def _rows_to_run(self, take: List[Tuple[int, int]]) -> List[Tuple[torch.Tensor, torch.Tensor, dict]]:
        """(tokens, mask, keywords) for the refill of each (slot, prompt index) of ``take``.  A registered prefix's K/V are copied into the slots HERE,
        one copy per handle (unless the initial fill's shared copy put them there), then the sampling table gets or loses the slots' entries,
        and only the rows after the prefix run: the caller begins at once, no frame step between any of it and the refill call."""
        copies: dict = {}                                           # id(handle) -> (handle, [slots]) still to copy
        for slot, i in take:
            handle = self.plan[i][1]
            if handle is not None and self.seeded.pop(slot, None) is not handle:
                copies.setdefault(id(handle), (handle, []))[1].append(slot)
        for handle, slots in copies.values():
            self.m.apply_prefix(handle, slots)
        parts = []
        for slot, i in take:
            (t, mk), (P, handle) = self.prompts[i], self.plan[i]
            if self.own[i] is not None:                             # after the prefix copies, immediately before the refill call
                self.m.set_slot_sampling([slot], *self.own[i])
                self.entries.add(slot)
            elif slot in self.entries:
                self.m.clear_slot_sampling([slot])
                self.entries.discard(slot)
            if self.warm[i]:
                P = self.warm[i]
                parts.append((t[P:], mk[P:], {"start": P}))
            else:
                parts.append((t[P:], mk[P:], {"start": P}) if handle is not None else (t, mk, {}))
        loads = [(self.sessions[i].device, slot) for slot, i in take if self.warm[i]]
        if loads:                                                   # all sessions of this refill call in one launch, immediately before it
            self.m.load_sessions([d for d, _ in loads], [slot for _, slot in loads])
        return parts

    def _report_order(self, cuts: List[Tuple[int, bool]]) -> List[Tuple[int, bool]]:
        return cuts                                                 # by slot


class _Stalling(LiveBatch):
    """``Model.refill_slot``: the batch waits while the whole prompt runs (~4 ms for 190 rows, > 8 ms for 1,334) and frame 0 comes back at
    once.  An all-zero frame 0, or a limit <= 0, is an empty utterance (generator.py:296) reported with slot -1; the slot takes the next."""

    def _vacated(self, slot: int) -> None:
        while self.pending:
            i = self.pending.popleft()
            (t, mk, kw), = self._rows_to_run([(slot, i)])
            f0 = self.m.refill_slot(slot, t, mk, *self.sampling, **kw).cpu()
            if self.limits[i] > 0 and not bool((f0 == 0).all()):
                self.slots[slot] = _Utterance(i, self.limits[i], self.g, [f0])
                return
            self._turn_over(i, slot, [])                            # (an empty reply is a turn too: the prompt's rows are in the slot)
            self.events.append((i, -1, _NO_FRAMES, True))

    def _feed(self, everything: bool) -> bool:
        while everything and self.free:     # (the initial fill; a slot that gets nothing there is not rewound)
            self._vacated(self.free.popleft())
        return False                        # later every vacated slot is refilled at once: with nobody generating nothing is left

    def _idle(self, vacated: List[int]) -> List[int]:
        return [s for s in vacated if self.slots[s] is None]        # out of prompts: rewound once

    def _report_order(self, cuts):
        return sorted(cuts, key=lambda c: c[1])                     # the ending slots last: each is followed by the empty utterances its refill met


class _BesideTheLoop(LiveBatch):
    """WITHOUT stalls: a retired slot's next prompt runs a few backbone layers after each frame step (Model.refill_begin / refill_advance: about
    ``budget`` = 600 prompt-row x layer units per step, i.e. 3 layers of a 190-row prompt = +8 % of a B = 32 step; measured: bench.py
    extras.config3.refill_beside_the_loop) while the other slots keep generating, and the new utterance's frame 0 is sampled by the batch's next
    frame step.  Until then the slot's rows are placeholders and are skipped.  Only the rows after a registered prefix count against the budget."""

    def __init__(self, *args, budget: int, group: int = 1, **kw):
        super().__init__(*args, **kw)
        self.budget, self.layers = budget, self.m.bb.num_layers
        # group > 1: free slots with prompts pending are refilled up to ``group`` at a time by ONE ragged prefill (Model.refill_group_begin /
        # refill_group_advance) -- slots that retire in the same block share one launch chain per layer instead of queueing with a handful
        # of rows each.  Requests with a seed of their own keep their codes whatever the group size (their draws do not depend on the schedule).
        self.group = max(1, min(int(group), 32))
        self.refilling: Optional[Tuple[List[Tuple[int, int]], int]] = None      # ([(slot, prompt index)], prompt rows to run), pending

    def _begin(self) -> None:
        """Takes up to ``group`` free slots with a pending prompt each -- as many as fit ``max_prefill_rows`` together, at least one -- and begins
        their refill: with ``group`` == 1 the slot's own (Model.refill_begin), else one group call, also for a single slot."""
        m = self.m
        cap = int(getattr(m, "max_prefill_rows", 0)) or (1 << 30)
        take: List[Tuple[int, int]] = []
        total = 0
        while self.free and self.pending and len(take) < self.group:
            i = self.pending[0]
            rows = int(self.prompts[i][0].shape[0]) - (self.warm[i] or (self.plan[i][0] if self.plan[i][1] is not None else 0))
            if take and total + rows > cap:
                break                                               # it waits for the next group
            take.append((self.free.popleft(), self.pending.popleft()))
            total += rows
        parts = self._rows_to_run(take)
        if self.group == 1:
            (t, mk, kw), = parts
            m.refill_begin(take[0][0], t, mk, **kw)
        else:
            m.refill_group_begin([slot for slot, _ in take], [(t, mk) for t, mk, _ in parts], starts=[kw.get("start", 0) for _, _, kw in parts])
        self.refilling = (take, total)

    def _feed(self, everything: bool) -> bool:
        """One bounded piece of refill work (``everything``: nobody is generating, so run whole prompts).  False: there was none."""
        m, fed = self.m, False
        advance = m.refill_advance if self.group == 1 else m.refill_group_advance
        while self.refilling is not None or (self.free and self.pending):
            if self.refilling is None:
                self._begin()
            take, rows = self.refilling
            # the per-step budget grows with the backlog: every slot that waits for a prompt is 1/B of the batch's throughput idle, and
            # the refill work is the same whenever it is done -- with nobody waiting the steps stay within ~8 % of an undisturbed one
            per_call = max(1, self.budget * (1 + len(self.free)) // max(rows, 1))
            if advance(self.layers if everything else min(per_call, self.layers)):
                first = m.num_frames()
                for slot, i in take:
                    self.slots[slot] = _Utterance(i, self.limits[i], first, [])
                self.refilling = None
            fed = True
            if not everything:
                break
        return fed

    def _vacated(self, slot: int) -> None:
        self.free.append(slot)

    def _idle(self, vacated: List[int]) -> List[int]:
        return list(self.free)                                      # they step as placeholders until a prompt takes them: rewound after every block


def _per_prompt(value, n: int, name: str):
    """(one value per prompt, whether ``value`` came as a sequence)."""
    if isinstance(value, (list, tuple)):
        if len(value) != n:
            raise ValueError(f"{name}: one value, or one per prompt")
        return list(value), True
    return [value] * n, False


def per_prompt_sampling(n: int, temperature, topk, seed):
    """``temperature`` / ``topk``: one value or one per prompt; ``seed``: None or one optional int per prompt.  Returns the scalars every frame
    step gets (the first prompt's where sequences were given) and, per prompt, ``(temperature, topk, seed)`` where the prompt has values of
    its own -- with sequences every prompt has, else only one with a seed -- or None."""
    temps, t_seq = _per_prompt(temperature, n, "temperature")
    ks, k_seq = _per_prompt(topk, n, "topk")
    seeds = [None] * n if seed is None else list(seed)
    if len(seeds) != n:
        raise ValueError("seed: None, or one optional int per prompt")
    temps, ks = [float(t) for t in temps], [int(k) for k in ks]
    if any(not t > 0 for t in temps) or any(k < 1 for k in ks):
        raise ValueError("temperature must be > 0 and topk >= 1")
    seeds = [None if s is None else int(s) for s in seeds]
    if not n:
        return (temperature, topk), []
    scalars = (temps[0] if t_seq else temperature, ks[0] if k_seq else topk)
    every = t_seq or k_seq
    own = [(temps[i], ks[i], seeds[i]) if every or seeds[i] is not None else None for i in range(n)]
    return scalars, own


def live_batch(model, prompts, max_generation_len, temperature, topk, poll, max_batch, store, beside_the_loop, refill_row_layers, max_seq_len,
               seed=None, refill_group: int = 1, first_chunk_frames: Optional[int] = None, sessions=None):
    """``LiveBatch.run`` over ``prompts`` [(tokens (S_i,33), mask (S_i,33)), ...] with one length limit for all or one per prompt (a
    request's own max_audio_length_ms), refilling beside the loop where the model's frame steps of this batch size honour it.
    ``temperature`` / ``topk``: one value, or one per prompt; ``seed``: one optional int per prompt (``per_prompt_sampling``).
    ``refill_group``: how many free slots one refill beside the loop may take together (1: one at a time, today's calls exactly).
    ``first_chunk_frames``: ``LiveBatch``'s ``first_chunk`` (None: today's blocks exactly).  ``sessions``: ``LiveBatch``'s (None: none)."""
    (temperature, topk), own = per_prompt_sampling(len(prompts), temperature, topk, seed)
    limits = [int(max_generation_len)] * len(prompts) if isinstance(max_generation_len, (int, float)) else [int(x) for x in max_generation_len]
    if len(limits) != len(prompts):
        raise ValueError("max_generation_len: one value, or one per prompt")
    for (t, _), lim in zip(prompts, limits):
        if t.shape[0] >= max_seq_len - lim:
            raise ValueError(f"Inputs too long, must be below max_seq_len - max_generation_len: {max_seq_len - lim}")
    if not prompts:
        return
    B = min(max_batch, len(prompts))
    args = (model, prompts, limits, temperature, topk, poll, B, store, own if any(o is not None for o in own) else None)
    supported = getattr(model, "supports_refill_beside_the_loop", None)         # (a scripted model may lack it)
    beside = supported is not None and supported(B) and beside_the_loop
    if int(refill_group) < 1:
        raise ValueError("refill_group must be >= 1")
    kw = {} if first_chunk_frames is None else {"first_chunk": int(first_chunk_frames)}
    if sessions is not None and any(c is not None for c in sessions):
        kw["sessions"] = list(sessions)
    yield from (_BesideTheLoop(*args, budget=refill_row_layers, group=refill_group, **kw) if beside else _Stalling(*args, **kw)).run()


class SlotStreams:
    """The stream state of ``generate_many_stream``: each batch slot is one stream of a ``MimiStreamPool``; ``owner[slot]`` is the request
    whose audio the slot's stream carries, ``held[slot]`` its frames not decoded yet.  Decodes run on ``side`` (a HIP stream, or None).
    ``first`` = k (None: off, today's calls exactly): a request's first chunk goes out as soon as its slot holds k frames, and everything
    that is ready after a block -- full chunks, first chunks, the endings' remainders -- goes into ONE ragged pool call (``_ragged_calls``).
    ``resampler`` (None: 24 kHz fp32, today's calls exactly): a pool of at least ``slots`` resampler streams (``ResamplerPool``), slot = stream;
    every pool call's PCM goes through ONE ``resampler.feed`` on ``side``, ``final`` for the slots whose request it closes -- a request's last
    chunk carries the filter's tail, also when it is empty at 24 kHz.
    ``stretcher`` with ``speeds`` (None: no speed change, today's calls exactly): a pool of at least ``slots`` time-stretch streams
    (``TimeStretchPool``), slot = stream, and one speed factor or None per REQUEST; a slot is reset with its request's speed when the request
    takes it, and every pool call's PCM of the requests that have a speed goes through ONE ``stretcher.feed`` on ``side`` BEFORE the resampler,
    ``final`` for the slots whose request it closes -- the stretch's tail comes with the request's last chunk, also when that chunk is empty at
    24 kHz.  A request whose speed is None (or 1.0) never touches the stretcher.
    ``marker`` with ``marks`` (None: no watermark, today's calls exactly): a pool of at least ``slots`` watermark streams (``WatermarkPool``),
    slot = stream, and one five-byte key or None per REQUEST; a slot is reset with its request's key when the request takes it, and every pool
    call's PCM of the requests that have a key goes through ONE ``marker.feed`` on ``side`` AFTER the stretch and BEFORE the resampler,
    ``final`` for the slots whose request it closes -- an open block (only a stretch leaves one: a chunk of whole frames is whole blocks) comes
    through with the request's last chunk, also when that chunk is empty at 24 kHz.
    ``leveler`` with ``levels`` (None: no levelling, today's calls exactly): a pool of at least ``slots`` loudness streams (``LoudnessPool``),
    slot = stream, and one ``Level`` or None per REQUEST; a slot is reset with its request's ``Level`` when the request takes it, and every pool
    call's PCM of the requests that have one goes through ONE ``leveler.level_feed`` on ``side`` AFTER the stretch and BEFORE the watermark --
    the mark goes into the samples that leave -- ``final`` for the slots whose request it closes.  The leveler holds nothing back: a bare
    ending hands it the stretch's tail, as the marker's does.  A request whose level is None never touches the pool.
    ``limiter`` with ``limits`` (None: no limiting, today's calls exactly): a pool of at least ``slots`` limiter streams (``LimiterPool``),
    slot = stream, and one ``Limit`` or None per REQUEST; a slot is reset with its request's ``Limit`` when the request takes it, and every pool
    call's PCM of the requests that have one goes through ONE ``limiter.feed`` on ``side`` AFTER the leveler and BEFORE the watermark -- stretch,
    level, limit, mark, resample -- ``final`` for the slots whose request it closes.  The limiter holds its look-ahead back: those samples come
    with the request's last chunk, also when that chunk is empty at 24 kHz."""

    def __init__(self, pool, slots: int, size: int, side, device, first: Optional[int] = None, resampler=None, stretcher=None,
                 speeds: Optional[Sequence[Optional[float]]] = None, marker=None, marks: Optional[Sequence] = None, leveler=None,
                 levels: Optional[Sequence] = None, limiter=None, limits: Optional[Sequence] = None):
        self.pool, self.size, self.side, self.first, self.resampler = pool, size, side, first, resampler
        self.stretcher, self.speeds = stretcher, speeds
        self.marker, self.marks = marker, marks
        self.leveler, self.levels = leveler, levels
        self.limiter, self.limits = limiter, limits
        self.limit: list = [None] * slots                           # (limiter) the Limit of the request that holds the slot
        self.level: list = [None] * slots                           # (leveler) the Level of the request that holds the slot
        self.mark: List[Optional[Sequence[int]]] = [None] * slots    # (marker) the key of the request that holds the slot
        self.speed: List[Optional[float]] = [None] * slots          # (stretcher) the speed of the request that holds the slot
        self.started: List[bool] = [False] * slots                  # whether the slot's request has had a chunk (``first`` only)
        self.owner: List[Optional[int]] = [None] * slots
        self.held: List[List[torch.Tensor]] = [[] for _ in range(slots)]
        self.no_pcm = torch.empty(0, dtype=getattr(resampler, "out_dtype", torch.float32), device=device)

    def chunks(self, block: list) -> List[Tuple[int, torch.Tensor, torch.Tensor, bool]]:
        """One polled block (a slot carries at most one utterance in it) -> its chunks: a stream is reset when a new request takes its slot, all slots that
        hold ``size`` frames go into ONE pool call, finishing requests flush the rest grouped by length and close with ONE ``last`` chunk, maybe empty."""
        owner, held, pool = self.owner, self.held, self.pool
        out: List[Tuple[int, torch.Tensor, torch.Tensor, bool]] = []
        fresh, ending = [], []                                      # slots a new request took / whose request ends, in this block
        for i, slot, fr, last in block:
            if slot < 0:
                out.append((i, self.no_pcm, _NO_FRAMES, True))
                continue
            if owner[slot] != i:
                owner[slot], held[slot], self.started[slot] = i, [], False
                fresh.append(slot)
            held[slot].extend(fr.unbind(0))
            if last:
                ending.append(slot)
        calls: list = []                                            # (slots, their frames, their PCM (.., 1, samples)) per pool call

        def decode(slots: List[int], T: int) -> None:
            frames = torch.stack([torch.stack(held[s_][:T]) for s_ in slots]).to(torch.int32)      # (n, T, 32)
            for s_ in slots:
                del held[s_][:T]
            calls.append((slots, frames, pool.decode(slots, frames.permute(0, 2, 1))))

        tails: dict = {}                                            # (resampler) slot -> the tail of a request whose closing chunk is empty at 24 kHz
        with torch.inference_mode(), (torch.cuda.stream(self.side) if self.side is not None else contextlib.nullcontext()):
            if fresh:
                pool.reset(fresh)
                if self.resampler is not None:
                    self.resampler.reset(fresh)
                if self.stretcher is not None:
                    for s_ in fresh:
                        self.speed[s_] = self.speeds[owner[s_]]
                    if quick := [s_ for s_ in fresh if self.speed[s_] is not None]:
                        self.stretcher.reset(quick, [self.speed[s_] for s_ in quick])
                if self.leveler is not None:
                    for s_ in fresh:
                        self.level[s_] = self.levels[owner[s_]]
                    if even := [s_ for s_ in fresh if self.level[s_] is not None]:
                        self.leveler.level_reset(even, [self.level[s_] for s_ in even])
                if self.limiter is not None:
                    for s_ in fresh:
                        self.limit[s_] = self.limits[owner[s_]]
                    if peaks := [s_ for s_ in fresh if self.limit[s_] is not None]:
                        self.limiter.reset(peaks, [self.limit[s_] for s_ in peaks])
                if self.marker is not None:
                    for s_ in fresh:
                        self.mark[s_] = self.marks[owner[s_]]
                    if keyed := [s_ for s_ in fresh if self.mark[s_] is not None]:
                        self.marker.reset(keyed, [list(self.mark[s_]) for s_ in keyed])
            if self.first is not None:
                self._ragged_calls(ending, calls)
            while self.first is None and (full := [s_ for s_, h in enumerate(held) if len(h) >= self.size]):
                decode(full, self.size)
            for T in sorted({len(held[s_]) for s_ in ending} - {0}):
                decode([s_ for s_ in ending if len(held[s_]) == T], T)
            final = {s_: k for k, (slots, _, _) in enumerate(calls) for s_ in slots}   # the call that holds a slot's newest chunk
            if self.stretcher is not None:                          # ONE stretch call per pool call, and one for the empty closing chunks
                for k, (slots, frames, pcm) in enumerate(calls):
                    if quick := [j for j, s_ in enumerate(slots) if self.speed[s_] is not None]:
                        ys = self.stretcher.feed([slots[j] for j in quick], [pcm[j][0] for j in quick],
                                                 [slots[j] in ending and final[slots[j]] == k for j in quick])
                        pcm = [pcm[j] for j in range(len(slots))]
                        for j, y in zip(quick, ys):
                            pcm[j] = y.unsqueeze(0)
                        calls[k] = (slots, frames, pcm)
                if bare := [s_ for s_ in ending if s_ not in final and self.speed[s_] is not None]:
                    tails = dict(zip(bare, self.stretcher.feed(bare, [self.no_pcm.float()] * len(bare), True)))
            if self.leveler is not None:                            # ONE leveler call per pool call, and one for the empty closing chunks
                for k, (slots, frames, pcm) in enumerate(calls):
                    if even := [j for j, s_ in enumerate(slots) if self.level[s_] is not None]:
                        ys = self.leveler.level_feed([slots[j] for j in even], [pcm[j][0] for j in even],
                                                     [slots[j] in ending and final[slots[j]] == k for j in even])
                        pcm = [pcm[j] for j in range(len(slots))]
                        for j, y in zip(even, ys):
                            pcm[j] = y.unsqueeze(0)
                        calls[k] = (slots, frames, pcm)
                if bare := [s_ for s_ in ending if s_ not in final and self.level[s_] is not None]:
                    tails.update(zip(bare, self.leveler.level_feed(bare, [tails.get(s_, self.no_pcm.float()) for s_ in bare], True)))
            if self.limiter is not None:                            # ONE limiter call per pool call, and one for the empty closing chunks
                for k, (slots, frames, pcm) in enumerate(calls):
                    if peaks := [j for j, s_ in enumerate(slots) if self.limit[s_] is not None]:
                        ys = self.limiter.feed([slots[j] for j in peaks], [pcm[j][0] for j in peaks],
                                               [slots[j] in ending and final[slots[j]] == k for j in peaks])
                        pcm = [pcm[j] for j in range(len(slots))]
                        for j, y in zip(peaks, ys):
                            pcm[j] = y.unsqueeze(0)
                        calls[k] = (slots, frames, pcm)
                if bare := [s_ for s_ in ending if s_ not in final and self.limit[s_] is not None]:
                    tails.update(zip(bare, self.limiter.feed(bare, [tails.get(s_, self.no_pcm.float()) for s_ in bare], True)))
            if self.marker is not None:                            # ONE watermark call per pool call, and one for the empty closing chunks
                for k, (slots, frames, pcm) in enumerate(calls):
                    if keyed := [j for j, s_ in enumerate(slots) if self.mark[s_] is not None]:
                        ys = self.marker.feed([slots[j] for j in keyed], [pcm[j][0] for j in keyed],
                                              [slots[j] in ending and final[slots[j]] == k for j in keyed])
                        pcm = [pcm[j] for j in range(len(slots))]
                        for j, y in zip(keyed, ys):
                            pcm[j] = y.unsqueeze(0)
                        calls[k] = (slots, frames, pcm)
                if bare := [s_ for s_ in ending if s_ not in final and self.mark[s_] is not None]:
                    tails.update(zip(bare, self.marker.feed(bare, [tails.get(s_, self.no_pcm.float()) for s_ in bare], True)))
            if self.resampler is not None:                          # ONE resampler call per pool call, and one for the empty closing chunks
                for k, (slots, frames, pcm) in enumerate(calls):
                    rs = self.resampler.feed(slots, [pcm[j][0] for j in range(len(slots))], [s_ in ending and final[s_] == k for s_ in slots])
                    calls[k] = (slots, frames, [y.unsqueeze(0) for y in rs])
                if bare := [s_ for s_ in ending if s_ not in final]:
                    tails = dict(zip(bare, self.resampler.feed(bare, [tails.get(s_, self.no_pcm.float()) for s_ in bare], True)))
        if self.side is not None:
            self.side.synchronize()
        for k, (slots, frames, pcm) in enumerate(calls):
            out.extend((owner[s_], pcm[j][0], frames[j], s_ in ending and final[s_] == k) for j, s_ in enumerate(slots))
        for s_ in ending:
            if s_ not in final:                                     # nothing was left to decode: the closing chunk is empty (at 24 kHz)
                out.append((owner[s_], tails.get(s_, self.no_pcm), _NO_FRAMES, True))
            owner[s_] = None
        return out

    def _ragged_calls(self, ending: List[int], calls: list) -> None:
        """With ``first`` = k: ONE ``decode_ragged`` call takes every slot that holds a full chunk (``size`` frames), every slot whose request
        has had no chunk yet and holds at least k frames (its first chunk is ALL it holds, up to ``size``) and every ending slot with frames
        left (up to ``size``); a slot that then still holds something to send -- it held more than ``size`` -- goes into a further call."""
        held, size = self.held, self.size
        while True:
            take = [(s_, min(len(h), size)) for s_, h in enumerate(held)
                    if h and (len(h) >= size or s_ in ending or (not self.started[s_] and len(h) >= self.first))]
            if not take:
                return
            slots = [s_ for s_, _ in take]
            frames = [torch.stack(held[s_][:T]).to(torch.int32) for s_, T in take]             # each (T_i, 32)
            for s_, T in take:
                del held[s_][:T]
                self.started[s_] = True
            calls.append((slots, frames, self.pool.decode_ragged(slots, [f.t() for f in frames])))
