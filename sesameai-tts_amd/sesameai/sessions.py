"""Conversation sessions: a dialogue's backbone K/V carried from turn to turn in the model's paged session store (include/csm_hip.h
csm_session_*).  Host code only; the reference (sesameai/generator.py) re-runs the whole history for every reply.

A ``Conversation`` (``Generator.open_session()``) is what ``generate`` / ``generate_stream`` / ``generate_codes`` take as ``session=`` and
``generate_many`` / ``generate_many_stream`` / ``iter_codes_continuous`` as ``sessions=[...]``.  With a session a call's ``context`` (or prompt
rows) lists only what is NEW since the session's last turn, and the call is DEFINED to equal the cold call whose context is everything the
session was ever given plus, after each earlier reply, ``Segment(speaker, that reply's text, audio_codes=the generated codes)``.

Numerics: the rows of the generated frames were written by the decode-step kernels, a cold run writes them with the prompt kernels.  Session
and cold runs therefore agree to bf16 rounding in K/V and logits, not bit for bit; greedy codes agree bit for bit wherever the decision
margins exceed that gap (the decisive checkpoints of the tests).  Sampled runs are not comparable between the two ways (a refill that
finishes sooner lands its frame 0 on another global frame index, which is part of the Philox key).  A session never fails a request for
lack of pages: a session that loses its pages keeps its host mirror and runs its next turn cold from it.

Endless conversations (``Generator.open_session(on_full="forget")``): a session whose history would no longer fit drops its
oldest turns IN PLACE before the turn's prompt is built -- the pinned units (the voice prompt) stay, the oldest units after them fall out
(``Conversation.units`` / ``forget`` / ``forget_rows``).  Nothing is recomputed: the kept rows before the cut are untouched, the rows after
it move down in the pages and their keys are rotated back by the number of rows dropped (``Session.forget``: one launch, ahead of the
turn's load).  What such a call MEANS: a WARM turn after a forget is DEFINED as the oracle run on the cache edited that way; a COLD turn
(the first, or after an eviction) runs the trimmed mirror.  The two differ by more than rounding -- the kept rows after the cut attended to
the dropped ones when they were computed, and still carry that -- but give the same greedy codes on the decisive checkpoints; sampled runs
are not comparable, for the reason above."""
from typing import List, Optional, Sequence, Tuple

import torch

from .models import SessionPoolFull


def _frame_rows(frames: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """Generated frames (n, 32) as prompt rows (n, 33): the codes under an audio mask, what ``Generator._tokenize_audio`` makes of them."""
    n = frames.shape[0]
    t = torch.zeros(n, 33, dtype=torch.long)
    m = torch.zeros(n, 33, dtype=torch.bool)
    t[:, :-1] = frames.to(torch.long)
    m[:, :-1] = True
    return t, m


class Conversation:
    """One dialogue.  ``tokens`` / ``mask``: the host mirror of the history's rows (R, 33) -- every prompt row the session was given and
    every frame it generated, in order, i.e. the cold prompt up to the last generated frame; ``device``: its ``Model`` session (the pages);
    ``rows``: how many of the mirror's leading rows the pages hold (0: the next turn runs cold); ``turns``: replies so far; ``replies``:
    their codes (32, n) each.

    Which rows a turn leaves in the pages: a frame's row is written by the step that samples its successor.  With a prompt of P rows and n
    generated frames, an utterance that ended on a sampled EOS frame leaves P + n rows; one cut at its length limit leaves P + n - 1 and
    its last frame becomes the first row of the next turn's suffix.  The next prompt always continues with the all-zero EOS row that ends
    a context segment's audio, then the new segments, then the reply's text.
    A call that generates nothing because its length limit is <= 0 leaves the session as it was, and so does a stream that is abandoned
    before its last block."""

    def __init__(self, owner, device, on_full: str = "raise", pinned: int = 1):
        self._owner, self.device = owner, device
        self.on_full, self.pinned = on_full, int(pinned)
        self.forgets = 0                                        # forget_rows calls that dropped rows
        self.tokens = torch.zeros(0, 33, dtype=torch.long)
        self.mask = torch.zeros(0, 33, dtype=torch.bool)
        self.turns = 0
        self.replies: List[torch.Tensor] = []
        self._last: Tuple[int, int] = (0, 0)                    # (prompt rows, generated frames) of the last turn
        self.last_used = 0
        self.evictions = 0                                      # times this session lost its pages to another's save (or its own)

    @property
    def rows(self) -> int:
        return int(self.device.rows) if self.device is not None else 0

    def full_prompt(self, tokens: torch.Tensor, mask: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        """The cold prompt of the next turn: the mirror, the EOS row that closes the last reply's audio, then the new rows (S, 33)."""
        if self.device is None:
            raise ValueError("this conversation has been closed")
        dev = tokens.device
        parts_t, parts_m = [self.tokens.to(dev)], [self.mask.to(dev)]
        if self.turns:
            eos_t, eos_m = _frame_rows(torch.zeros(1, 32, dtype=torch.long))
            parts_t.append(eos_t.to(dev)); parts_m.append(eos_m.to(dev))
        parts_t.append(tokens.long()); parts_m.append(mask.bool())
        return torch.cat(parts_t, 0), torch.cat(parts_m, 0)

    def units(self) -> List[Tuple[int, int]]:
        """The mirror's rows as units [(first row, one past the last), ...]: split AFTER every all-zero audio row -- the EOS row that ends
        every segment's audio (a generated frame is never all zero: an all-zero frame ends generation).  A unit is thus one segment (its
        text rows, its audio, its EOS row); what follows the last EOS row is the OPEN unit: the last reply (with its text rows), whose EOS
        row only arrives with the next turn.  The open unit is listed last when it has rows; ``closed_units`` leaves it out."""
        out, at = [], 0
        for r in self._eos_rows().nonzero().flatten().tolist():
            out.append((at, r + 1))
            at = r + 1
        if at < self.tokens.shape[0]:
            out.append((at, int(self.tokens.shape[0])))
        return out

    def _eos_rows(self) -> torch.Tensor:
        return self.mask[:, :-1].all(1) & ~self.mask[:, -1] & (self.tokens == 0).all(1)

    def closed_units(self) -> List[Tuple[int, int]]:
        """``units`` without the open one."""
        eos = self._eos_rows()
        return [(a, b) for a, b in self.units() if bool(eos[b - 1])]

    def plan_forget(self, new_rows: int, limit: int, max_seq_len: int) -> Tuple[int, int]:
        """What ``on_full="forget"`` drops before a turn of ``new_rows`` new rows and a reply limit of ``limit`` frames: (first unit, number
        of units) -- the SMALLEST number of consecutive closed units from unit ``pinned`` on after which mirror + EOS row + new rows <
        max_seq_len - limit.  (pinned, 0): nothing needs to go, the session raises on a full window, or no number of units makes the
        prompt fit (then nothing is dropped and the call raises the ValueError it always raised).  Never the pinned units, never the open
        unit, never the new rows.  No side effects."""
        room = int(max_seq_len) - int(limit)
        need = int(self.tokens.shape[0]) + (1 if self.turns else 0) + int(new_rows)
        if self.on_full != "forget" or need < room:
            return self.pinned, 0
        closed = self.closed_units()
        for n in range(1, len(closed) - self.pinned + 1):
            if need - (closed[self.pinned + n - 1][1] - closed[self.pinned][0]) < room:
                return self.pinned, n
        return self.pinned, 0

    def forget(self, first_unit: int, n_units: int, busy: Sequence["Conversation"] = ()) -> None:
        """Drops the closed units [first_unit, first_unit + n_units) (``units``): ``forget_rows`` in whole units."""
        closed = self.closed_units()
        if n_units < 1 or first_unit < 0 or first_unit + n_units > len(closed):
            raise ValueError(f"forget: units [{first_unit}, {first_unit + n_units}) are not closed units of this conversation ({len(closed)} closed)")
        self.forget_rows(closed[first_unit][0], closed[first_unit + n_units - 1][1], busy)

    def forget_rows(self, a: int, b: int, busy: Sequence["Conversation"] = ()) -> None:
        """Drops the history's rows [a, b) in place: the mirror is cut, the (prompt rows, frames) that ``truncate_last`` uses move down by
        b - a, and -- if the pages hold rows from ``a`` on -- the pages drop the same rows (``Session.forget``: rows after the cut move down,
        keys rotated back by b - a; enqueued now, i.e. ahead of the next turn's load).  The range must lie within the rows before the last
        reply's frames.  When the pool is too short for the fresh pages the least recently used conversation outside ``busy`` loses its
        pages, as in ``turn_over``; with none left this session goes cold itself.  A cold session only trims its mirror.  The next turn then
        is: warm -- the cache edited this way (the module's docstring); cold -- the trimmed mirror."""
        a, b = int(a), int(b)
        P, n = self._last
        if self.device is None:
            raise ValueError("this conversation has been closed")
        if not 0 <= a <= b <= (P if self.turns else 0):
            raise ValueError(f"forget_rows: 0 <= a <= b <= {P if self.turns else 0} (the rows before the last reply's frames) required")
        if a == b:
            return
        self.tokens = torch.cat([self.tokens[:a], self.tokens[b:]], 0)
        self.mask = torch.cat([self.mask[:a], self.mask[b:]], 0)
        self._last = (P - (b - a), n)
        self.forgets += 1
        held = self.rows
        if held <= a:
            return                                              # cold, or the pages end before the cut
        if held < b:
            self.device.truncate(a)
            return
        while True:
            try:
                self.device.forget(a, b)
                return
            except SessionPoolFull:
                victim = self._owner._evictable([*busy, self])
                if victim is None:
                    victim = self
                victim.device.truncate(0)
                victim.evictions += 1
                if victim is self:
                    return

    def turn_over(self, model, slot: int, tokens: torch.Tensor, mask: torch.Tensor, frames: torch.Tensor, limit: int, busy: Sequence["Conversation"]) -> None:
        """The turn whose full prompt was (tokens, mask) (P, 33) and whose frames (n, 32) are all handed out has ended in batch slot ``slot``:
        the mirror takes the prompt and the frames, the pages take the slot's new rows (``Model.save_session``: stream-ordered, between frame
        steps).  When the pool is short the least recently used conversation outside ``busy`` (the running call's) loses its pages; with
        none left to evict this one goes cold itself."""
        P, n = int(tokens.shape[0]), int(frames.shape[0])
        ft, fm = _frame_rows(frames.cpu())
        self.tokens = torch.cat([tokens.detach().cpu().long(), ft], 0)
        self.mask = torch.cat([mask.detach().cpu().bool(), fm], 0)
        self.turns += 1
        self.replies.append(frames.cpu().to(torch.int32).t().contiguous())
        self._last = (P, n)
        self._owner._touch(self)
        rows = P + n if n < limit else P + n - 1
        while True:
            try:
                model.save_session(self.device, slot, rows)
                return
            except SessionPoolFull:
                victim = self._owner._evictable([*busy, self])
                if victim is None:
                    victim = self
                victim.device.truncate(0)
                victim.evictions += 1
                if victim is self:
                    return

    def truncate_last(self, frames_kept: int) -> None:
        """Barge-in: the listener heard only the first ``frames_kept`` frames of the last reply.  The mirror and the pages are cut to them;
        the next turn equals the cold call whose context holds only those frames of that reply."""
        P, n = self._last
        k = int(frames_kept)
        if not self.turns or not 0 <= k <= n:
            raise ValueError(f"truncate_last: 0 .. {n} frames of the last reply can be kept")
        self.tokens, self.mask = self.tokens[:P + k], self.mask[:P + k]
        self.replies[-1] = self.replies[-1][:, :k]
        self._last = (P, k)
        if self.rows > P + k:
            self.device.truncate(P + k)

    def close(self) -> None:
        """Returns the pages to the pool."""
        if self.device is not None:
            self.device.close()
            self.device = None
            self._owner._forget(self)


class ConversationSet:
    """The conversations opened on one Generator, for the eviction order (least recently used first)."""

    def __init__(self):
        self.open: List[Conversation] = []
        self.clock = 0

    def new(self, device, on_full: str = "raise", pinned: int = 1) -> Conversation:
        c = Conversation(self, device, on_full, pinned)
        self.open.append(c)
        self._touch(c)
        return c

    def _touch(self, c: Conversation) -> None:
        self.clock += 1
        c.last_used = self.clock

    def _forget(self, c: Conversation) -> None:
        self.open = [x for x in self.open if x is not c]

    def _evictable(self, busy: Sequence[Conversation]) -> Optional[Conversation]:
        held = [c for c in self.open if c.rows > 0 and not any(c is b for b in busy)]
        return min(held, key=lambda c: c.last_used) if held else None


def check_sessions(sessions, n: int) -> list:
    """``sessions`` of a call with ``n`` requests -> a list of n (Conversation or None); at most one request per session."""
    sessions = [None] * n if sessions is None else list(sessions)
    if len(sessions) != n:
        raise ValueError("sessions: None, or one (Conversation or None) per request")
    live = [c for c in sessions if c is not None]
    if len({id(c) for c in live}) != len(live):
        raise ValueError("sessions: at most one request per session in one call")
    return sessions


def make_room(sessions: Sequence[Optional[Conversation]], new_rows: Sequence[int], limits: Sequence[int], max_seq_len: int) -> None:
    """Before the full prompts of one call are built: every ``on_full="forget"`` session of the call drops what its turn needs dropped
    (``Conversation.plan_forget``).  All or nothing over the call: if a request would still be too long afterwards nothing is forgotten --
    the call is about to raise its ValueError and must leave the sessions as they were."""
    plans = [None if c is None else c.plan_forget(r, lim, max_seq_len) for c, r, lim in zip(sessions, new_rows, limits)]
    for c, r, lim, p in zip(sessions, new_rows, limits, plans):
        rows = r if c is None else c.tokens.shape[0] + (1 if c.turns else 0) + r
        if c is not None and p[1]:
            closed = c.closed_units()
            rows -= closed[p[0] + p[1] - 1][1] - closed[p[0]][0]
        if rows >= max_seq_len - lim:
            return
    busy = [c for c in sessions if c is not None]
    for c, p in zip(sessions, plans):
        if c is not None and p[1]:
            c.forget(p[0], p[1], busy)
