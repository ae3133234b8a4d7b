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
lack of pages: a session that loses its pages keeps its host mirror and runs its next turn cold from it."""
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

    def __init__(self, owner, device):
        self._owner, self.device = owner, device
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

    def new(self, device) -> Conversation:
        c = Conversation(self, device)
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
