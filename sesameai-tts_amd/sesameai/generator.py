"""Generation driver with the reference's surface (reference: sesameai/generator.py).

``Segment``, ``Generator.generate`` / ``generate_stream`` / ``_tokenize_*`` and ``load_csm_1b``
keep the reference's names, argument meaning and error behaviour; the frame loop itself runs on
the GPU from on-device state (one hipGraph replay per 80 ms frame) and the host only polls the
EOS flag every few frames instead of synchronising on every frame (generator.py:285).
"""
from __future__ import annotations

import contextlib
import os
import queue
import struct
import threading
import time
from dataclasses import dataclass
from typing import Callable, Generator as PyGenerator, List, Optional, Sequence, Tuple, Union

import torch

from .live_batch import SlotStreams, live_batch, per_prompt_sampling
from .models import Model, ModelArgs, csm_1b_args
from .sessions import Conversation, ConversationSet, check_sessions, make_room

FRAME_MS = 80                     # generator.py:257
MAX_SEQ_LEN = 2048                # generator.py:276


def _frames_for(max_audio_length_ms):
    """A length limit in ms, or one per request, in frames."""
    return int(max_audio_length_ms / FRAME_MS) if isinstance(max_audio_length_ms, (int, float)) else [int(x / FRAME_MS) for x in max_audio_length_ms]


# Distinct unencoded context clips from which prompt building uses the ragged encode (MimiCodec.encode_many) instead of one ``encode``
# per clip: the measured break-even (docs/experiments/encode_many.md).
ENCODE_MANY_MIN_CLIPS = 2


@dataclass
class Segment:
    """reference: sesameai/generator.py:16-21.  ``audio`` is (num_samples,) @ 24 kHz.
    Extension: ``audio_codes`` (32, T) may carry pre-computed Mimi codes, and ``text`` may be
    a list of token ids, so prompts can be built without the gated tokenizer / Mimi encoder; ``sample_rate`` (None: 24 kHz) is the rate
    ``audio`` comes at, fp32 or int16 -- a foreign rate is resampled on the device before Mimi sees it (the reference's callers do it with
    torchaudio first, tts_service.py:161-166)."""
    speaker: int
    text: Union[str, Sequence[int]]
    audio: Optional[torch.Tensor] = None
    audio_codes: Optional[torch.Tensor] = None
    sample_rate: Optional[int] = None


def load_llama3_tokenizer(path: Optional[str] = None):
    """reference: sesameai/generator.py:24-38 -- Llama-3.2-1B tokenizer with the bos/eos
    TemplateProcessing.  Loads a local ``tokenizer.json`` (no hub access here)."""
    from tokenizers import Tokenizer
    from tokenizers.processors import TemplateProcessing
    path = path or os.environ.get("CSM_TOKENIZER_JSON")
    if not path or not os.path.exists(path):
        return None
    tok = Tokenizer.from_file(path)
    bos, eos = "<|begin_of_text|>", "<|end_of_text|>"
    bos_id, eos_id = tok.token_to_id(bos), tok.token_to_id(eos)
    tok.post_processor = TemplateProcessing(
        single=f"{bos}:0 $A:0 {eos}:0",
        pair=f"{bos}:0 $A:0 {eos}:0 {bos}:1 $B:1 {eos}:1",
        special_tokens=[(bos, bos_id), (eos, eos_id)])
    return tok


class _FirstBlockGate:
    """Handed by ``generate_stream`` to ``_frame_blocks``: the frame loop binds the action that queues the block after the
    first, the stream calls ``release()`` once the first chunk's decode has been submitted.  One gate per stream -- two
    streams on one Generator cannot release each other's blocks, and an abandoned stream leaves nothing installed."""

    def __init__(self) -> None:
        self._action: Optional[Callable[[], None]] = None

    def bind(self, action: Optional[Callable[[], None]]) -> None:
        self._action = action

    def release(self) -> None:
        action, self._action = self._action, None
        if action is not None:
            action()


class Generator:
    """reference: sesameai/generator.py:41-300."""
    # the live batch's settings, for callers to assign; class-level so that a Generator assembled without __init__ (tests, tools) has them
    refill_beside_the_loop = True              # refill a few layers per frame step where the model supports it (sesameai/live_batch.py) ...
    refill_row_layers = 600                    # ... about this many prompt-row x layer units per step
    _stream_pools: Optional[dict] = None       # {(slots, chunk frames): MimiStreamPool} of generate_many_stream, made on first use and kept
    _conversations: Optional[ConversationSet] = None   # the sessions opened on this Generator (open_session), made on first use
    segment_meters: dict = {}                  # request -> (4,) int64 {S, n, peak, hops} on the device, of the last run that levelled
    _finisher = None                           # generate_segments' SegmentFinisher (sesameai/finish.py), made on first use and kept

    def __init__(self, model: Model, audio_tokenizer=None, text_tokenizer=None, max_batch_size: int = 1):
        self._model = model
        self._model.setup_caches(max_batch_size)
        self._max_batch = max_batch_size
        self._text_tokenizer = text_tokenizer if text_tokenizer is not None else load_llama3_tokenizer()
        self._audio_tokenizer = audio_tokenizer
        self.sample_rate = getattr(audio_tokenizer, "sample_rate", 24_000)
        self.device = model.device
        self._stream_buffer_size = 10          # generator.py:61
        self._eos_poll = 8                     # frames launched between EOS polls
        self._mimi_stream = None               # side HIP stream for Mimi in generate_stream / generate_many_stream (_side_stream)

    def warm_up(self, temperature: float = 0.7, topk: int = 30, also=((0.8, 40), (0.9, 50))) -> None:
        """One short synthetic utterance through the streaming path and the whole-utterance path.  Everything a process does once --
        torch's first device kernels of each kind, the HIP module load, the frame-step graph's capture (for THIS temperature / top-k),
        the Mimi chunk graph, the side stream -- is paid here instead of by the first request: measured on an MI355X
        (tools/dbg/first_chunk_breakdown.py), the first utterance of a process took 164 ms to its first chunk against 30 ms for
        every later one.  ``load_csm_1b`` calls it (CSM_NO_WARMUP=1 skips it); the reference has no counterpart.
        ``also``: further (temperature, top-k) pairs whose frame-step graphs are captured too -- the engine keeps 4 captured steps per
        handle (csm_frame_step), and the reference's callers use 0.8 / 40 (tts_service.py:266) and 0.9 / 50 (:175) beside 0.7 / 30."""
        if self._audio_tokenizer is None or self.device.type != "cuda":
            return
        g = torch.Generator().manual_seed(0)
        ctx = [Segment(speaker=0, text=[11] * 40, audio_codes=torch.randint(0, 2048, (32, 60), generator=g))]
        n = 2 * self._stream_buffer_size + 2
        for _ in self.generate_stream([11] * 12, 0, ctx, max_audio_length_ms=n * FRAME_MS, temperature=temperature, topk=topk):
            pass
        self.generate([11] * 12, 0, ctx, max_audio_length_ms=4 * FRAME_MS, temperature=temperature, topk=topk)
        for (t, k) in also or ():
            if (float(t), int(k)) != (float(temperature), int(topk)):
                self._model.step(1, float(t), int(k))       # one more frame on the warm-up's state: captures that key's graph
        self._model._kv_prompt = None                       # the synthetic prompt is nobody's prefix
        # the warm-up's frames advanced the Philox step counter: put the noise stream back where a process without the warm-up
        # (CSM_NO_WARMUP=1) has it, so the two produce the same audio for the same requests
        self._model.seed(getattr(self._model, "_seed_value", 0))
        torch.cuda.synchronize(self.device)

    # -- prompt assembly (generator.py:63-109) ------------------------------------------------
    def _text_ids(self, text: Union[str, Sequence[int]], speaker: int) -> List[int]:
        if not isinstance(text, str):
            return [int(t) for t in text]
        if self._text_tokenizer is None:
            raise RuntimeError("no text tokenizer: set CSM_TOKENIZER_JSON to a local Llama-3.2 tokenizer.json "
                               "or pass token ids instead of a string")
        enc = self._text_tokenizer.encode(f"[{speaker}]{text}")
        return list(enc.ids if hasattr(enc, "ids") else enc)

    def _tokenize_text_segment(self, text, speaker: int) -> Tuple[torch.Tensor, torch.Tensor]:
        ids = self._text_ids(text, speaker)
        frame = torch.zeros(len(ids), 33).long()
        mask = torch.zeros(len(ids), 33).bool()
        frame[:, -1] = torch.tensor(ids, dtype=torch.long)
        mask[:, -1] = True
        return frame.to(self.device), mask.to(self.device)

    def _tokenize_audio(self, audio: Optional[torch.Tensor], codes: Optional[torch.Tensor] = None, sample_rate: Optional[int] = None):
        if codes is None:
            assert audio is not None and audio.ndim == 1, "Audio must be single channel"
            if self._audio_tokenizer is None or not hasattr(self._audio_tokenizer, "encode"):
                raise RuntimeError("no Mimi encoder available: pass Segment.audio_codes")
            kw = {} if sample_rate is None else {"sample_rate": sample_rate}
            codes = self._audio_tokenizer.encode(audio.to(self.device).unsqueeze(0).unsqueeze(0), **kw)[0]
        codes = codes.to(self.device).long()
        eos = torch.zeros(codes.size(0), 1, dtype=torch.long, device=self.device)     # all-zero EOS frame
        codes = torch.cat([codes, eos], dim=1)
        frame = torch.zeros(codes.size(1), 33, dtype=torch.long, device=self.device)
        mask = torch.zeros(codes.size(1), 33, dtype=torch.bool, device=self.device)
        frame[:, :-1] = codes.transpose(0, 1)
        mask[:, :-1] = True
        return frame, mask

    def _tokenize_segment(self, segment: Segment, encoded: Optional[dict] = None) -> Tuple[torch.Tensor, torch.Tensor]:
        t, tm = self._tokenize_text_segment(segment.text, segment.speaker)
        codes = segment.audio_codes
        if codes is None and encoded:
            codes = encoded.get(id(segment.audio))          # (the Segment itself is left as it came)
        a, am = self._tokenize_audio(segment.audio, codes, **({} if segment.sample_rate is None else {"sample_rate": segment.sample_rate}))
        return torch.cat([t, a], dim=0), torch.cat([tm, am], dim=0)

    def _encode_contexts(self, contexts: Sequence[List[Segment]]) -> dict:
        """{id(audio tensor): codes (32, T)} of every context Segment that has ``audio`` and no ``audio_codes``, from ragged encode
        calls (``MimiCodec.encode_many``: all clips, whatever their lengths, in one launch chain; the codes are bit for bit those of
        the per-segment ``encode``).  A tensor that several segments or requests share (the same object) is encoded once.  Empty --
        the segments then go through today's per-segment ``encode`` calls -- for a codec without ``encode_many`` and for fewer than
        ENCODE_MANY_MIN_CLIPS distinct clips.  A segment's ``sample_rate`` goes with its clip (``encode_many(.., sample_rates=..)``)."""
        tok = self._audio_tokenizer
        if tok is None or not hasattr(tok, "encode_many"):
            return {}
        clips: dict = {}
        rates: dict = {}
        for ctx in contexts:
            for seg in ctx:
                if seg.audio is not None and seg.audio_codes is None and id(seg.audio) not in clips:
                    assert seg.audio.ndim == 1, "Audio must be single channel"
                    clips[id(seg.audio)] = seg.audio
                    rates[id(seg.audio)] = seg.sample_rate
        if len(clips) < max(2, ENCODE_MANY_MIN_CLIPS):
            return {}
        kw = {} if all(r is None for r in rates.values()) else {"sample_rates": list(rates.values())}
        return dict(zip(clips.keys(), tok.encode_many(list(clips.values()), **kw)))

    def _build_prompts(self, texts: Sequence, speakers: Sequence[int], contexts: Sequence[List[Segment]]):
        """The prompts of several requests; their unencoded context audio goes through the Mimi encoder together (_encode_contexts)."""
        encoded = self._encode_contexts(contexts)
        return [self._build_prompt(t, sp, ctx, encoded) for t, sp, ctx in zip(texts, speakers, contexts)]

    def _build_prompt(self, text, speaker: int, context: List[Segment], encoded: Optional[dict] = None):
        if encoded is None:
            encoded = self._encode_contexts([context])
        toks, masks = [], []
        for seg in context:
            t, m = self._tokenize_segment(seg, encoded)
            toks.append(t); masks.append(m)
        t, m = self._tokenize_text_segment(text, speaker)
        toks.append(t); masks.append(m)
        return torch.cat(toks, 0).long().to(self.device), torch.cat(masks, 0).bool().to(self.device)

    def open_turn_streams(self, n: int, chunk_frames: int = 10, sample_rate: Optional[int] = None, vad=None, pre_roll_ms: int = 200,
                          post_roll_ms: int = 200, features=None):
        """``n`` spoken turns encoded while they are spoken (sesameai/turns.py): ``feed`` / ``pump`` as the microphones deliver, then
        ``finish(sid, speaker, text)`` gives the ``Segment`` of the turn, its codes bit for bit those of ``Segment(audio=the turn)``.
        ``sample_rate`` (None: 24 kHz, today's calls exactly): the microphones' rate; ``feed`` then takes fp32 or int16 at that rate and a
        pool of ``n`` resampler streams (sesameai/resample.py) follows the turns in front of the encoder.
        ``vad`` (None: today's calls exactly): ``True`` for a pool of ``n`` voice-activity streams (sesameai/vad.py), or such a pool; the
        streams then listen all the time, a turn starts ``pre_roll_ms`` before the detected START and ends ``post_roll_ms`` after the
        detected END, and ``poll_events`` says when.
        ``features`` (None: today's calls exactly, nothing imported): ``True`` or 80 for a ``TurnFeatures`` of ``n`` streams with 80 mel
        bands (sesameai/mel.py), 128 for 128 bands, or such an object; ``take_features(sid)`` then has each ended turn's Whisper input."""
        from .turns import TurnStreams
        tok = self._audio_tokenizer
        if tok is None or not hasattr(tok, "open_encode_streams"):
            raise RuntimeError("no Mimi encoder with encode streams available: pass Segment.audio_codes")
        pool = tok.open_encode_streams(n, max_chunk_frames=chunk_frames)
        kw = {}
        if features is not None and features is not False:
            if features is True or (isinstance(features, int) and features in (80, 128)):
                from .mel import TurnFeatures
                features = TurnFeatures(n, src_rate=self.sample_rate, n_mels=80 if features is True else int(features), device=self.device)
            kw["features"] = features
        if vad is not None and vad is not False:
            if vad is True:
                from .vad import VadPool
                vad = VadPool(n, device=self.device)
            kw.update({"vad": vad, "pre_roll": int(pre_roll_ms) * self.sample_rate // 1000, "post_roll": int(post_roll_ms) * self.sample_rate // 1000})
        if sample_rate is None or int(sample_rate) == self.sample_rate:
            return TurnStreams(pool, tok.args.hop, chunk_frames, **kw)
        from .resample import ResamplerPool
        return TurnStreams(pool, tok.args.hop, chunk_frames, resampler=ResamplerPool(int(sample_rate), self.sample_rate, n, device=self.device), **kw)

    # -- prefix store: a voice prompt's K/V computed once, copied into any slot ----------------------
    def _store(self) -> list:
        """[(tokens (P,33) zeroed where masked, mask (P,33), handle)] of the registered prefixes.  The list lives on the model:
        ``Model.prefill_prompt`` (B = 1) reads it too, and ``Model.setup_caches`` empties it with the handle the snapshots came from."""
        if not hasattr(self._model, "stored_prefixes"):               # (a scripted model of the host-logic tests)
            self._model.stored_prefixes = []
        return self._model.stored_prefixes

    def cache_prefix(self, context, mask: Optional[torch.Tensor] = None):
        """Registers a prompt prefix -- a voice's context ``List[Segment]``, or its rows ``(tokens (P,33), mask (P,33))`` -- with
        the prefix store: the rows are prefilled once (call it while no generation is running: it resets the caches), their backbone
        K/V snapshotted (Model.capture_prefix), and every later request whose prompt starts with them -- ``generate``,
        ``generate_stream``, ``generate_many``, ``generate_many_stream``, ``iter_codes_continuous`` -- copies the snapshot into its
        slot and prefills only the rows after it.  The results are bit-identical to running the whole prompt (in prompt mode a row's
        K/V do not depend on the rows that share its call).  Returns the handle (``.rows``, ``.bytes``); ``drop_prefix`` frees it."""
        if mask is None:
            toks, masks = zip(*[self._tokenize_segment(seg) for seg in context])
            tokens, mask = torch.cat(toks, 0), torch.cat(masks, 0)
        else:
            tokens = context
        tokens, mask = tokens.to(self.device).long(), mask.to(self.device).bool()
        if tokens.dim() != 2 or tokens.shape[0] < 1 or tokens.shape[0] >= MAX_SEQ_LEN:
            raise ValueError(f"a prefix is (P,33) rows with 1 <= P < {MAX_SEQ_LEN}")
        m = self._model
        m.reset_caches()
        m.prefill_prompt(tokens.unsqueeze(0), mask.unsqueeze(0))
        handle = m.capture_prefix(0, int(tokens.shape[0]))
        self._store().append((torch.where(mask, tokens, torch.zeros_like(tokens)), mask, handle))
        return handle

    def drop_prefix(self, handle) -> None:
        """Forgets a registered prefix and frees its snapshot."""
        st = self._store()
        st[:] = [e for e in st if e[2] is not handle]
        handle.destroy()

    @property
    def prefixes(self) -> list:
        """Handles of the registered prefixes, oldest first."""
        return [e[2] for e in self._store()]

    # -- conversation sessions: a dialogue's K/V carried from turn to turn (sesameai/sessions.py) -------
    def open_session_store(self, pages: int, page_rows: int = 64) -> None:
        """The model's pool of K/V pages for ``open_session`` (Model.open_session_store): ``pages`` pages of ``page_rows`` rows, 2 MB each
        at CSM-1B with 64 rows; a 1,334-row history holds 21 of them.  Once per Generator."""
        self._model.open_session_store(pages, page_rows)

    def open_session(self, on_full: str = "raise", pinned: int = 1) -> Conversation:
        """A new conversation (sesameai/sessions.py ``Conversation``) for ``session=`` / ``sessions=``: every turn's call then lists only the
        segments that are new since the last one, the history's K/V are loaded from the session's pages and only the new rows are
        prefilled.  The results are those of the cold call with the whole history as its context, to bf16 rounding (see the module's
        docstring); ``truncate_last`` covers barge-in, ``close`` returns the pages.  Needs ``open_session_store``.

        ``on_full``: what a turn does whose history + new rows no longer fit below MAX_SEQ_LEN - max_generation_len.  "raise": the
        ``ValueError`` of every entry point, as without sessions.  "forget": an endless conversation -- before the turn's full prompt is built
        (``generate``, ``generate_stream``, ``generate_codes``, ``generate_many``, ``generate_many_stream``, ``iter_codes_continuous``) the
        session drops the smallest number of consecutive closed units (segments: ``Conversation.units``) from unit ``pinned`` on that makes
        the prompt fit; the first ``pinned`` units (the voice prompt), the open unit (the last reply) and the new rows are never dropped,
        and if the prompt still does not fit nothing is dropped and the ValueError is raised.  The pages drop the rows in place, ahead of
        the turn's load (``Session.forget``); nothing is recomputed.  A WARM turn after a forget is DEFINED as the oracle run on the cache
        edited that way (kept rows before the cut untouched; later rows moved down, their keys rotated back by the rows dropped); a COLD
        turn (the first, or after an eviction) runs the trimmed history.  The two differ by more than rounding, because kept rows have
        attended to dropped ones; they give the same greedy codes on the decisive checkpoints; sampled runs are not comparable."""
        if on_full not in ("raise", "forget") or int(pinned) < 0:
            raise ValueError('open_session: on_full is "raise" or "forget", pinned >= 0')
        if self._conversations is None:
            self._conversations = ConversationSet()
        return self._conversations.new(self._model.open_session(), on_full, int(pinned))

    # -- the frame loop -----------------------------------------------------------------------
    def _frame_blocks(self, prompt_tokens: torch.Tensor, prompt_mask: torch.Tensor, max_generation_len: int,
                      temperature: float, topk: int, poll: int, gate: Optional["_FirstBlockGate"] = None,
                      session: Optional[Conversation] = None) -> PyGenerator[torch.Tensor, None, None]:
        """Yields the generated frames in blocks [n][B][32] int32 (CPU) of about ``poll`` frames, cut at EOS for
        B == 1.  The NEXT block's frame steps are already enqueued on the GPU when a block is yielded, so whatever
        the consumer does with it (Mimi decode on another stream, playback) overlaps the language model.

        ``gate`` (streaming only): time to the first audio.  With a gate the FIRST block (frame 0 + poll - 1 steps) is handed
        out before anything else is queued -- its consumer (the first Mimi decode) then has the GPU to itself instead of
        squeezing between frame steps whose persistent launches occupy every CU (first 10-frame chunk: 38.8 -> 31 ms) -- and
        the second block is queued when the consumer calls ``gate.release()`` (generate_stream: right after submitting the
        first decode, BEFORE the chunk goes to the user) or, at the latest, when it asks for the next block.  Without a gate
        (generate_codes: nobody decodes between blocks) every block, the first included, is followed at once by the next.
        ``session`` (B == 1; the prompt is the session's FULL prompt, ``Conversation.full_prompt``): the rows its pages hold are loaded into
        slot 0 and only the rows after them run; when the last block has been read the slot's new rows are saved, before it is yielded."""
        B = prompt_tokens.shape[0]
        m = self._model
        m.reset_caches()
        self.last_eos_at = torch.full((B,), -1, dtype=torch.int32)
        if max_generation_len <= 0:
            return
        if session is not None and session.rows > 0:
            m.load_sessions([session.device], [0])          # (slot 0 is nobody's cached prompt now) immediately before the suffix's prefill
            m.prefill_prompt(prompt_tokens, prompt_mask, start=session.rows)
        else:
            m.prefill_prompt(prompt_tokens, prompt_mask)    # reuses the cached KV of a shared voice-prompt prefix
        m.depth(B, temperature, topk, commit=True)
        launched, delivered = 1, 0
        kept: List[torch.Tensor] = []                       # a session's turn: every frame handed out, for its mirror

        def enqueue(want: int) -> int:
            n = max(min(want, max_generation_len - launched), 0)
            for _ in range(n):
                m.step(B, temperature, topk)
            return n

        launched += enqueue(poll - 1)
        held = gate is not None                 # the block after the first waits for the consumer's go

        def open_gate() -> None:
            nonlocal launched, held
            if held:
                held = False
                launched += enqueue(poll)

        if gate is not None:
            gate.bind(open_gate)
        try:
            while True:
                upto = launched
                fr, eos = m.read_frames(B, delivered, upto - delivered)          # waits for the frames launched so far
                self.last_eos_at = eos
                done = bool((eos >= 0).all()) or launched >= max_generation_len
                if done:
                    held = False                                                # nothing more to launch
                elif not held:
                    launched += enqueue(poll)                                   # keep the GPU busy before handing out
                if B == 1 and eos[0] >= 0:
                    fr = fr[: max(int(eos[0]) - delivered, 0)]
                delivered = upto
                if session is not None:
                    kept.append(fr[:, 0])
                    if done:                                                    # the last block has been read: the slot's new rows go to the pages
                        session.turn_over(m, 0, prompt_tokens[0], prompt_mask[0], torch.cat(kept), max_generation_len, [session])
                if fr.shape[0]:
                    yield fr
                if done:
                    return
                open_gate()                                                     # a consumer that never released is released now
        finally:
            held = False
            if gate is not None:
                gate.bind(None)

    @torch.inference_mode()
    def generate_codes(self, prompt_tokens: torch.Tensor, prompt_mask: torch.Tensor, max_generation_len: int,
                       temperature: float, topk: int, on_frames: Optional[Callable[[torch.Tensor], None]] = None,
                       poll: Optional[int] = None, session: Optional[Conversation] = None) -> torch.Tensor:
        """prompt (S,33) or (B,S,33) -> frames [n][B][32] int32 (CPU), cut at each sequence's EOS
        for B == 1 (the reference is batch-1: generator.py:47).  For B > 1 all sequences run
        ``max_generation_len`` frames unless every one hit EOS; the caller trims with ``last_eos_at``.
        ``session`` (one sequence): the prompt holds only the rows that are NEW since the session's last turn (``open_session``)."""
        if prompt_tokens.dim() == 2:
            prompt_tokens, prompt_mask = prompt_tokens.unsqueeze(0), prompt_mask.unsqueeze(0)
        if session is not None:
            prompt_tokens, prompt_mask = self._session_prompt(session, prompt_tokens, prompt_mask, max_generation_len)
        B, S, _ = prompt_tokens.shape
        max_context_len = MAX_SEQ_LEN - max_generation_len
        if S >= max_context_len:
            raise ValueError(f"Inputs too long, must be below max_seq_len - max_generation_len: {max_context_len}")
        blocks = []
        for fr in self._frame_blocks(prompt_tokens, prompt_mask, max_generation_len, temperature, topk, poll or self._eos_poll, session=session):
            if on_frames is not None:
                on_frames(fr)
            blocks.append(fr)
        return torch.cat(blocks) if blocks else torch.empty(0, B, 32, dtype=torch.int32)

    @staticmethod
    def _session_prompt(session: Conversation, tokens: torch.Tensor, mask: torch.Tensor, limit: int) -> Tuple[torch.Tensor, torch.Tensor]:
        """(1,S,33) new rows -> the session's full prompt (1,S',33); an ``on_full="forget"`` session first drops what the turn needs dropped."""
        if tokens.shape[0] != 1:
            raise ValueError("session=: one sequence per call (sessions= of generate_many takes several)")
        make_room([session], [tokens.shape[1]], [limit], MAX_SEQ_LEN)
        t, mk = session.full_prompt(tokens[0], mask[0])
        return t.unsqueeze(0), mk.unsqueeze(0)

    @torch.inference_mode()
    def iter_codes_continuous(self, prompts: Sequence[Tuple[torch.Tensor, torch.Tensor]], max_generation_len: Union[int, Sequence[int]],
                              temperature: Union[float, Sequence[float]], topk: Union[int, Sequence[int]], poll: Optional[int] = None,
                              seed: Optional[Sequence[Optional[int]]] = None, refill_group: int = 1,
                              sessions: Optional[Sequence[Optional[Conversation]]] = None) -> PyGenerator[Tuple[int, torch.Tensor], None, None]:
        """Any number of prompts [(tokens (S_i,33), mask (S_i,33)), ...] of any lengths through a batch of ``max_batch_size``
        slots that is kept FULL: an utterance that reaches its all-zero EOS frame (generator.py:285) or the length limit is
        retired and its slot re-prefilled with the next prompt (Model.refill_slot) while the other slots keep generating --
        their frames are bit-identical to an undisturbed run.  Yields ``(index of the prompt, frames [n_i][32] int32 CPU)`` as
        each utterance FINISHES (cut at its EOS like the reference's batch-1 loop, or at ``max_generation_len`` -- one limit for
        all prompts or one per prompt), so a long run hands its results out as it
        goes.  ``temperature`` / ``topk``: one value for all prompts or one per prompt; ``seed``: one optional int per prompt -- a prompt with
        a seed of its own yields the same frames whichever slot it takes and whatever the batch did before (Model.set_slot_sampling).  There is no limit on the total number of frame steps: the engine's frame history is a ring (include/csm_hip.h,
        csm_read_frames) and every block of ``poll`` steps is read before the next one is launched.
        ``sessions``: one ``Conversation`` or None per prompt, at most one prompt per session (else ValueError): such a prompt holds only the
        rows that are NEW since its session's last turn; the pages of all sessions of a refill group are loaded by one call immediately
        before the group's refill, and a finished turn's rows are saved between frame steps (``open_session``).  None: today's calls exactly."""
        parts: dict = {}
        for block in self._iter_blocks_continuous(prompts, max_generation_len, temperature, topk, poll, seed=seed, refill_group=refill_group,
                                                  **({} if sessions is None else {"sessions": sessions})):
            for i, _slot, frames, last in block or ():
                parts.setdefault(i, []).append(frames)
                if last:
                    got = parts.pop(i)
                    yield i, (got[0] if len(got) == 1 else torch.cat(got))

    @torch.inference_mode()
    def _iter_blocks_continuous(self, prompts: Sequence[Tuple[torch.Tensor, torch.Tensor]], max_generation_len: Union[int, Sequence[int]],
                                temperature: Union[float, Sequence[float]], topk: Union[int, Sequence[int]], poll: Optional[int] = None,
                                seed: Optional[Sequence[Optional[int]]] = None, refill_group: int = 1,
                                first_chunk_frames: Optional[int] = None, sessions: Optional[Sequence[Optional[Conversation]]] = None,
                                slots: Optional[int] = None):
        """The incremental form of ``iter_codes_continuous`` (same loop, same model calls in the same order): per polled block it
        yields a list of ``(index of the prompt, batch slot, that utterance's NEW frames [k][32] int32 CPU, last)`` -- ``last`` with
        the frames that complete the utterance (possibly none); an utterance that is empty before it ever holds a slot has slot -1.
        In between it yields ``None`` each time a block's frame steps have just been queued and before it waits for them: the
        moment for a consumer to start work that should run beside those steps (generate_many_stream's Mimi decode).
        The scheduler is sesameai/live_batch.py; ``refill_beside_the_loop`` / ``refill_row_layers`` choose and tune how slots are refilled;
        ``first_chunk_frames``: its short blocks while a request waits for its first chunk (None: every block is ``poll`` steps);
        ``slots``: use no more than this many of the batch's slots (None: all ``max_batch_size``)."""
        per_prompt_sampling(len(prompts), temperature, topk, seed)          # (a wrong length or a bad value raises before the model is touched)
        kw = {}
        if sessions is not None:                                            # the sessions' prompts become their full prompts
            kw["sessions"] = sessions = check_sessions(sessions, len(prompts))
            limits = [int(max_generation_len)] * len(prompts) if isinstance(max_generation_len, (int, float)) else [int(x) for x in max_generation_len]
            if len(limits) == len(prompts):                                 # (a wrong length is live_batch's ValueError) on_full="forget": make room first
                make_room(sessions, [t.shape[0] for t, _ in prompts], limits, MAX_SEQ_LEN)
            prompts = [(t, mk) if c is None else c.full_prompt(t, mk) for (t, mk), c in zip(prompts, sessions)]
        yield from live_batch(self._model, prompts, max_generation_len, temperature, topk, poll or self._eos_poll,
                              self._max_batch if slots is None else min(self._max_batch, int(slots)),
                              self._store(), self.refill_beside_the_loop, self.refill_row_layers, MAX_SEQ_LEN, seed=seed, refill_group=refill_group,
                              first_chunk_frames=first_chunk_frames, **kw)

    def generate_codes_continuous(self, prompts: Sequence[Tuple[torch.Tensor, torch.Tensor]], max_generation_len: int,
                                  temperature: Union[float, Sequence[float]], topk: Union[int, Sequence[int]], poll: Optional[int] = None,
                                  seed: Optional[Sequence[Optional[int]]] = None, refill_group: int = 1,
                                  sessions: Optional[Sequence[Optional[Conversation]]] = None) -> List[torch.Tensor]:
        """``iter_codes_continuous`` collected: each prompt's frames [n_i][32] int32 (CPU), in the order of ``prompts``."""
        results: List[torch.Tensor] = [torch.empty(0, 32, dtype=torch.int32) for _ in prompts]
        for i, frames in self.iter_codes_continuous(prompts, max_generation_len, temperature, topk, poll, seed=seed, refill_group=refill_group,
                                                    **({} if sessions is None else {"sessions": sessions})):
            results[i] = frames
        return results

    def generate_many(self, texts: Sequence, speakers: Sequence[int], contexts: Sequence[List[Segment]], max_audio_length_ms=90_000,
                      temperature: Union[float, Sequence[float]] = 0.7, topk: Union[int, Sequence[int]] = 30,
                      seed: Optional[Sequence[Optional[int]]] = None, refill_group: int = 1,
                      sessions: Optional[Sequence[Optional[Conversation]]] = None, finish=None,
                      on_result: Optional[Callable[[int, torch.Tensor], None]] = None, speed=None, watermark=None) -> List[torch.Tensor]:
        """``generate`` for a list of requests through the continuously refilled batch: one audio tensor per request
        (``max_audio_length_ms``, ``temperature``, ``topk``: one value, or one per request; ``seed``: one optional int per request;
        ``sessions``: one ``Conversation`` or None per request -- the context of a request with a session lists only the NEW segments).
        ``finish`` (None: the calls described above, exactly): a ``SegmentFinish``, or one per request -- the result is then what
        ``generate_segments`` returns for these prompts, finished int16 segments on the device, and ``on_result(i, pcm)`` fires as each
        request completes.
        ``speed`` (None: the calls described above, exactly): a speech-rate factor in 0.5 .. 2.0, or one (or None) per request -- each decoded
        clip goes through the device time stretch (sesameai/stretch.py) before anything else sees it; with ``finish`` all clips that end in
        a block share ONE stretch call.
        ``watermark`` (None: the calls described above, exactly): True or "device" for the public CSM key, or a five-byte key -- each clip
        carries the device watermark (sesameai/watermarking.py) after the stretch; with ``finish`` all clips that end in a block share ONE
        embed call in front of the finish."""
        max_generation_len = _frames_for(max_audio_length_ms)
        prompts = self._build_prompts(texts, speakers, contexts)
        if finish is not None:
            if sessions is not None:
                raise ValueError("finish= with sessions=: not supported")
            return self.generate_segments(prompts, max_generation_len, temperature, topk, finish, seed=seed, refill_group=refill_group,
                                          on_result=on_result, **({} if speed is None else {"speed": speed}),
                                          **({} if watermark is None else {"watermark": watermark}))
        if on_result is not None:
            raise ValueError("on_result= needs finish=")
        speeds = self._speeds(speed, len(prompts))
        key = self._mark_key(watermark)
        out: List[torch.Tensor] = [torch.tensor([]) for _ in prompts]
        for i, frames in self.iter_codes_continuous(prompts, max_generation_len, temperature, topk, seed=seed, refill_group=refill_group,
                                                    **({} if sessions is None else {"sessions": sessions})):
            if frames.shape[0]:                                       # decoded as each utterance finishes, not at the end
                out[i] = self._decode_frames(frames.unsqueeze(1))
                if speeds[i] is not None:
                    out[i] = self._stretch_clip(out[i], speeds[i])
                if key is not None:
                    out[i] = self._mark_clip(out[i], key)
        return out

    @staticmethod
    def _speeds(speed, n: int) -> List[Optional[float]]:
        """``speed=`` as one checked factor or None per request (None for all without importing anything: today's calls exactly)."""
        if speed is None:
            return [None] * n
        from .stretch import per_request
        return per_request(speed, n)

    @staticmethod
    def _stretch_clip(audio: torch.Tensor, speed: float) -> torch.Tensor:
        """One decoded clip through a one-shot device time stretch (sesameai/stretch.py)."""
        from .stretch import stretch
        return stretch([audio], speed)[0] if audio.numel() else audio

    @staticmethod
    def _mark_key(watermark) -> Optional[List[int]]:
        """``watermark=`` as a checked five-byte key, or None (None without importing anything: today's calls exactly)."""
        if watermark is None:
            return None
        from .watermarking import key_of
        return key_of(watermark)

    @staticmethod
    def _mark_clip(audio: torch.Tensor, key: List[int]) -> torch.Tensor:
        """One clip through a one-shot device watermark embed (sesameai/watermarking.py)."""
        from .watermarking import embed
        return embed([audio], key)[0] if audio.numel() else audio

    def generate_segments(self, prompts: Sequence[Tuple[torch.Tensor, torch.Tensor]], max_generation_len: Union[int, Sequence[int]],
                          temperature: Union[float, Sequence[float]], topk: Union[int, Sequence[int]], finish,
                          seed: Optional[Sequence[Optional[int]]] = None, refill_group: int = 1,
                          post: Optional[Callable[[torch.Tensor], torch.Tensor]] = None,
                          on_result: Optional[Callable[[int, torch.Tensor], None]] = None, slots: Optional[int] = None,
                          speed=None, watermark=None) -> List[torch.Tensor]:
        """Prompts [(tokens (S_i,33), mask (S_i,33)), ...] through the continuously refilled batch, each result a FINISHED segment: int16 on
        the device, peak-normalised, with lead and tail silence and fades (``finish``: a ``SegmentFinish`` for all prompts, or one per
        prompt; sesameai/finish.py) -- what ``tts_service.TTS.generate_audio_segment`` makes of a sentence, bit for bit, without the float32
        copy to the host.  After each polled block the utterances that ended in it are decoded, and ALL their clips are finished by ONE
        ``SegmentFinisher.finish`` call; decode and finish run on the Mimi side stream and are submitted right after the next block's frame
        steps have been queued (``generate_many_stream``'s backlog pattern), so the language model never waits for them.
        ``post(audio) -> audio`` runs on each non-empty decoded clip before it is finished (the watermark hook); ``on_result(i, pcm)``
        fires as each request completes; an utterance with no frames still yields its lead and tail silence.  ``max_generation_len``,
        ``temperature``, ``topk``, ``seed``, ``refill_group``: as for ``iter_codes_continuous``; ``slots``: use no more than this
        many of the batch's slots (None: all of them).  Returns the segments in the order of ``prompts``.
        ``speed`` (None: the calls described above, exactly): a speech-rate factor in 0.5 .. 2.0, or one (or None) per prompt: the decoded
        clips that end in a block go through ONE ``stretch`` call (sesameai/stretch.py), then ``post``, then the ONE finish call -- the
        stretch acts on the decoded fp32 clip, so lead and tail silence keep their lengths.
        ``watermark`` (None: the calls described above, exactly): True, "device" or a five-byte key -- the block's non-empty clips go through
        ONE device embed call (sesameai/watermarking.py) after the stretch and ``post``, in front of the finish: the mark that replaces the
        host ``post`` hook, so a segment stays on the device between decode and finish.
        A ``SegmentFinish`` with ``loudness=`` (LUFS) brings its clip to that integrated loudness instead of to its own peak: the block's
        clips are metered on the device (sesameai/loudness.py) in front of the ONE finish call, and ``segment_meters[i]`` keeps what the
        meter said of request i, on the device.  Without it the calls are those described above, exactly."""
        from .finish import SegmentFinisher, per_clip
        how = per_clip(finish, len(prompts))
        self.segment_meters = {}
        speeds = self._speeds(speed, len(prompts))
        key = self._mark_key(watermark)
        if self._finisher is None:
            self._finisher = SegmentFinisher(self.device)
        side = self._side_stream()
        results: List[Optional[torch.Tensor]] = [None] * len(prompts)
        parts: dict = {}
        no_audio = torch.empty(0, dtype=torch.float32, device=self.device)

        def finish_block(block: list) -> None:
            done = []                                               # (request, its frames) of the utterances that end in this block
            for i, _slot, frames, last in block:
                parts.setdefault(i, []).append(frames)
                if last:
                    got = parts.pop(i)
                    done.append((i, got[0] if len(got) == 1 else torch.cat(got)))
            if not done:
                return
            with torch.inference_mode(), (torch.cuda.stream(side) if side is not None else contextlib.nullcontext()):
                clips = []
                for i, frames in done:
                    audio = self._decode_frames(frames.unsqueeze(1)) if frames.shape[0] else no_audio
                    clips.append(post(audio) if post is not None and audio.numel() and speeds[i] is None else audio)
                if quick := [j for j, (i, _) in enumerate(done) if speeds[i] is not None and clips[j].numel()]:
                    from .stretch import stretch                    # ONE stretch call for the block's clips, then post, then the finish
                    for j, y in zip(quick, stretch([clips[j] for j in quick], [speeds[done[j][0]] for j in quick])):
                        clips[j] = post(y) if post is not None else y
                if key is not None and (heard := [j for j, c in enumerate(clips) if c.numel()]):
                    from .watermarking import embed                 # ONE embed call for the block's clips, then the finish
                    for j, y in zip(heard, embed([clips[j] for j in heard], key)):
                        clips[j] = y
                pcm = self._finisher.finish(clips, [how[i] for i, _ in done], self.sample_rate)
                if len(done) <= 64 and any(how[i].loudness is not None for i, _ in done):   # what the meter said of each clip, kept on the device
                    for j, (i, _) in enumerate(done):
                        self.segment_meters[i] = self._finisher.last_meter[j]
            if side is not None:
                side.synchronize()
            for (i, _), seg in zip(done, pcm):
                results[i] = seg
                if on_result is not None:
                    on_result(i, seg)

        backlog: List[list] = []                                    # polled blocks whose utterances are still to be decoded and finished
        for block in self._iter_blocks_continuous(prompts, max_generation_len, temperature, topk, seed=seed, refill_group=refill_group,
                                                  **({} if slots is None else {"slots": slots})):
            if block is not None:
                backlog.append(block)
                continue
            while backlog:                                          # the next block's steps are queued: decode and finish beside them
                finish_block(backlog.pop(0))
        while backlog:
            finish_block(backlog.pop(0))
        return results

    def generate_many_stream(self, texts: Sequence, speakers: Sequence[int], contexts: Sequence[List[Segment]], max_audio_length_ms=90_000,
                             temperature: Union[float, Sequence[float]] = 0.7, topk: Union[int, Sequence[int]] = 30,
                             seed: Optional[Sequence[Optional[int]]] = None, refill_group: int = 1, first_chunk_frames: Optional[int] = None,
                             sessions: Optional[Sequence[Optional[Conversation]]] = None,
                             out_sample_rate: Optional[int] = None, out_dtype: Optional[torch.dtype] = None, speed=None,
                             watermark=None, loudness=None, limiter=None) -> PyGenerator[Tuple[int, torch.Tensor, torch.Tensor, bool], None, None]:
        """``generate_many`` that hands out audio as it comes into existence: yields ``(request index, pcm chunk (samples,) fp32,
        the chunk's frames [t][32] int32 CPU, last)`` for every request while the continuously refilled batch keeps generating.
        Each batch slot is one stream of a ``MimiStreamPool`` (reset when a new utterance takes the slot); after every polled block
        all slots that hold ``_stream_buffer_size`` undecoded frames are decoded by ONE pool call, and finishing utterances flush
        their remaining 1..9 frames grouped by equal length.  The decode runs on the Mimi side stream and is submitted right after
        the next block's frame steps have been queued, so the language model never waits for it.  Every request ends with exactly
        one ``last=True`` chunk, which is empty (0 samples, 0 frames) when no frames remain -- an utterance whose first frame is EOS
        yields just that.  All other chunks are ``_stream_buffer_size`` frames.
        The streams are STATEFUL: the chunks of one request, concatenated, are the whole-clip decode of its frames (what
        ``generate_many`` returns for them).  ``generate_stream`` differs: it keeps the reference's stateless 10-frame chunks.
        ``temperature`` / ``topk`` / ``seed``: as for ``generate_many``.
        ``first_chunk_frames`` = k, 1 <= k < ``_stream_buffer_size`` (None, the default: the calls described above, exactly): a request's
        first audio does not wait for a whole block.  While some request has had no chunk yet, a block of frame steps ends as soon as that
        request has k frames queued, and after every block ONE ragged pool call (``MimiStreamPool.decode_ragged``) takes every slot with a
        full chunk, every slot whose request has had no chunk and holds at least k frames -- its first chunk is all it holds -- and the
        endings' remainders.  So chunk lengths become: the first >= k frames (or the whole request, if shorter), later ones
        ``_stream_buffer_size``, the last whatever remains; everything else above holds, and a request's chunks concatenated are still its
        whole-clip decode, bit for bit what the uniform calls give.  The Philox key of a sampled frame holds the global frame index, so --
        as with ``refill_group`` -- the sampled codes of requests WITHOUT a seed of their own may differ between None and k (the shorter
        blocks see the retirements at other steps); requests with their own seed, and greedy runs, give the same codes for every k.
        ``sessions``: as for ``generate_many``.
        ``out_sample_rate`` / ``out_dtype`` (None, None: fp32 at 24 kHz, the calls described above exactly): the rate and the format
        (torch.float32 or torch.int16) the caller's device wants.  Each slot is then also one stream of a ``ResamplerPool``
        (sesameai/resample.py), reset when a new request takes the slot, and each pool call's PCM goes through ONE resampler call on the
        side stream.  A request's chunks, concatenated, are bit for bit ``resample`` of its concatenated 24 kHz chunks; the filter's tail
        comes with the request's last chunk -- also with the closing chunk that is empty at 24 kHz -- so a chunk's length is no longer
        1920 samples a frame.  ``out_dtype`` other than fp32 needs a foreign ``out_sample_rate`` (the conversion is the resampler's).
        ``speed`` (None: the calls described above exactly): a speech-rate factor in 0.5 .. 2.0, or one (or None) per request.  Each slot is
        then also one stream of a ``TimeStretchPool`` (sesameai/stretch.py), reset with the request's speed when the request takes the slot,
        and each pool call's PCM goes through ONE stretch call on the side stream, BEFORE the resampler.  A request's chunks, concatenated,
        are bit for bit ``stretch`` of its concatenated ``speed=None`` chunks (with ``out_sample_rate``: ``resample`` of that); the stretch
        holds back up to 1,280 samples, which come with the request's last chunk -- also with a closing chunk that is empty at 24 kHz.  A
        request whose speed is None or 1.0 never touches the stretcher: its chunks are those of a run without ``speed``.
        ``watermark`` (None: the calls described above exactly): True or "device" for the public CSM key, or a five-byte key.  Each slot is
        then also one stream of a ``WatermarkPool`` (sesameai/watermarking.py), reset with the key when a request takes the slot, and each
        pool call's PCM goes through ONE embed call on the side stream, AFTER the stretch and BEFORE the resampler.  A request's chunks,
        concatenated, are bit for bit ``embed`` of its concatenated ``watermark=None`` chunks; a chunk of whole frames is whole blocks and
        lags by nothing, behind a stretch the mark holds back fewer than 1920 samples, which come with the request's last chunk.
        ``loudness`` (None: the calls described above exactly, nothing imported): a target in LUFS or a ``Level`` (sesameai/loudness.py), or
        one (or None) per request.  Each slot is then also one leveler stream of a ``LoudnessPool``, reset with the request's ``Level`` when
        the request takes the slot, and each pool call's PCM goes through ONE ``level_feed`` on the side stream, AFTER the stretch and BEFORE
        the watermark.  The leveler is causal and holds nothing back: chunk lengths stay what they were, and a request's chunks,
        concatenated, are bit for bit ``level`` of its concatenated ``loudness=None`` chunks.  The gain starts at ``Level.start_gain`` and
        follows the gated loudness measured so far by at most 1 / 2^slew_shift per 100 ms, under the ceiling.  A request whose level is None
        never touches the pool: its chunks are those of a run without ``loudness``.
        ``limiter`` (None: the calls described above exactly, nothing imported): True for the default ``Limit`` (sesameai/limiter.py), a
        ``Limit``, or one of these (or None) per request.  Each slot is then also one stream of a ``LimiterPool``, reset with the request's
        ``Limit`` when the request takes the slot, and each pool call's PCM goes through ONE limiter ``feed`` on the side stream, AFTER the
        leveler and BEFORE the watermark: stretch, level, limit, mark, resample.  The limiter holds back ``Limit.lookahead`` samples
        (``Limit(true_peak=True)``, which makes the ceiling hold for the 4x oversampled waveform too: 8 more), which come with the request's last chunk -- also with a closing chunk that is empty at 24 kHz; a request's chunks, concatenated, are bit
        for bit ``limit`` of its concatenated ``limiter=None`` chunks.  With ``loudness`` given too, a request that has both gets the pair
        of ``sesameai.limiter.paired``: its leveler runs ``Limit.headroom_shift`` doublings lower under a 0 dB ceiling and the limiter is
        driven by as many, so an onset that the leveler alone would clamp is brought down ahead of its peak.  A request whose limit is None
        never touches the pool."""
        size = self._stream_buffer_size
        if first_chunk_frames is not None and not 1 <= int(first_chunk_frames) < size:
            raise ValueError(f"first_chunk_frames must be None or 1 .. {size - 1}")
        first = None if first_chunk_frames is None else int(first_chunk_frames)
        codec = self._audio_tokenizer
        if codec is None or not hasattr(codec, "open_streams"):
            raise RuntimeError("generate_many_stream needs a Mimi codec with stream pools (MimiCodec.open_streams)")
        max_generation_len = _frames_for(max_audio_length_ms)
        with torch.inference_mode():
            prompts = self._build_prompts(texts, speakers, contexts)
        if not prompts:
            return
        B = min(self._max_batch, len(prompts))
        if self._stream_pools is None:
            self._stream_pools = {}
        if (B, size) not in self._stream_pools:
            self._stream_pools[(B, size)] = codec.open_streams(B, max_chunk_frames=size)
        kw = {} if first is None else {"first": first}
        if out_sample_rate is not None and int(out_sample_rate) != self.sample_rate:
            from .resample import ResamplerPool
            key = ("resampler", B, int(out_sample_rate), out_dtype or torch.float32)
            if key not in self._stream_pools:
                self._stream_pools[key] = ResamplerPool(self.sample_rate, int(out_sample_rate), B, device=self.device, out_dtype=out_dtype or torch.float32)
            kw["resampler"] = self._stream_pools[key]
        elif out_dtype is not None and out_dtype != torch.float32:
            raise ValueError("out_dtype without out_sample_rate: convert the 24 kHz chunks yourself")
        speeds = self._speeds(speed, len(prompts))
        if any(v is not None for v in speeds):
            from .stretch import TimeStretchPool
            if ("stretcher", B) not in self._stream_pools:
                self._stream_pools[("stretcher", B)] = TimeStretchPool(B, device=self.device)
            kw["stretcher"], kw["speeds"] = self._stream_pools[("stretcher", B)], speeds
        limits = None
        if limiter is not None:
            from .limiter import LimiterPool, paired, per_request_limits
            limits = per_request_limits(limiter, len(prompts))
        if loudness is not None:
            from .loudness import LoudnessPool, per_request_levels
            levels = per_request_levels(loudness, len(prompts))
            if limits is not None:                                  # a request with both: the leveler lower by the headroom, the limiter driven by it
                both = [paired(lv, lm) if lv is not None and lm is not None else (lv, lm) for lv, lm in zip(levels, limits)]
                levels, limits = [lv for lv, _ in both], [lm for _, lm in both]
            if any(v is not None for v in levels):
                if ("leveler", B) not in self._stream_pools:
                    self._stream_pools[("leveler", B)] = LoudnessPool(B, device=self.device)
                kw["leveler"], kw["levels"] = self._stream_pools[("leveler", B)], levels
        if limits is not None and any(v is not None for v in limits):
            if ("limiter", B) not in self._stream_pools:
                self._stream_pools[("limiter", B)] = LimiterPool(B, device=self.device)
            kw["limiter"], kw["limits"] = self._stream_pools[("limiter", B)], limits
        if (key := self._mark_key(watermark)) is not None:
            from .watermarking import WatermarkPool, default_secret
            at = ("marker", B, default_secret(key))
            if at not in self._stream_pools:
                self._stream_pools[at] = WatermarkPool(B, at[2], device=self.device)
            kw["marker"], kw["marks"] = self._stream_pools[at], [key] * len(prompts)
        streams = SlotStreams(self._stream_pools[(B, size)], B, size, self._side_stream(), self.device, **kw)
        backlog: List[list] = []                                    # polled blocks whose audio is still to be decoded
        for block in self._iter_blocks_continuous(prompts, max_generation_len, temperature, topk, size, seed=seed, refill_group=refill_group,
                                                  **({} if first is None else {"first_chunk_frames": first}),
                                                  **({} if sessions is None else {"sessions": sessions})):
            if block is not None:
                backlog.append(block)
                continue
            while backlog:                                          # the next block's steps are queued: decode beside them
                yield from streams.chunks(backlog.pop(0))
        while backlog:
            yield from streams.chunks(backlog.pop(0))

    def _side_stream(self):
        """The HIP stream Mimi decodes on beside the frame steps, made on first use; None on a CPU device (the host-logic tests)."""
        if torch.device(self.device).type != "cuda":
            return None
        if self._mimi_stream is None:
            self._mimi_stream = torch.cuda.Stream(device=self.device)
        return self._mimi_stream

    def _decode_frames(self, frames: torch.Tensor) -> torch.Tensor:
        """frames [n][1][32] -> audio (n*1920,) (reference: _decode_frames, generator.py:111-117)."""
        if frames.shape[0] == 0:
            return torch.tensor([])
        if self._audio_tokenizer is None:
            raise RuntimeError("no Mimi decoder attached to this Generator")
        codes = frames.to(self.device).permute(1, 2, 0).contiguous()          # (B, 32, T)
        return self._audio_tokenizer.decode(codes).squeeze(0).squeeze(0)

    def generate_stream(self, text, speaker: int, context: List[Segment], max_audio_length_ms: float = 90_000,
                        temperature: float = 0.7, topk: int = 30,
                        on_chunk_generated: Optional[Callable[[torch.Tensor], None]] = None,
                        session: Optional[Conversation] = None) -> PyGenerator[torch.Tensor, None, None]:
        """reference: generator.py:119-210 -- yields audio every ``_stream_buffer_size`` frames as soon as it exists,
        each buffer decoded statelessly like the reference.  Mimi runs on its own HIP stream while the frame steps
        of the next buffer (already enqueued) run on the caller's stream.  There is no ``speed=`` here: the chunks are the reference's
        stateless ones, and a stretch needs a stream's state (``generate_many_stream`` has it; ``generate(.., speed=)`` stretches the clip).
        ``session``: ``context`` lists only the segments that are NEW since the session's last turn (``open_session``)."""
        max_generation_len = int(max_audio_length_ms / FRAME_MS)
        with torch.inference_mode():
            tokens, mask = self._build_prompt(text, speaker, context)
        if tokens.dim() == 2:
            tokens, mask = tokens.unsqueeze(0), mask.unsqueeze(0)
        if session is not None:
            tokens, mask = self._session_prompt(session, tokens, mask, max_generation_len)
        if tokens.shape[1] >= MAX_SEQ_LEN - max_generation_len:
            raise ValueError(f"Inputs too long, must be below max_seq_len - max_generation_len: {MAX_SEQ_LEN - max_generation_len}")
        side = self._side_stream()
        pending: List[torch.Tensor] = []
        size = self._stream_buffer_size

        def decode(n: int) -> torch.Tensor:
            buf = torch.stack(pending[:n]); del pending[:n]
            if side is None:
                with torch.inference_mode():
                    return self._decode_frames(buf)
            with torch.inference_mode(), torch.cuda.stream(side):
                pcm = self._decode_frames(buf)
            side.synchronize()
            return pcm

        gate = _FirstBlockGate()
        blocks = self._frame_blocks(tokens, mask, max_generation_len, temperature, topk, size, gate=gate, session=session)
        while True:
            with torch.inference_mode():
                fr = next(blocks, None)
            if fr is None:
                break
            pending.extend(fr.unbind(0))
            while len(pending) >= size:
                chunk = decode(size)
                gate.release()                   # the first chunk is decoded: queue the next block before the user gets this one
                if on_chunk_generated:
                    on_chunk_generated(chunk)
                yield chunk
        if pending:
            chunk = decode(len(pending))
            if on_chunk_generated:
                on_chunk_generated(chunk)
            yield chunk

    @torch.inference_mode()
    def generate(self, text, speaker: int, context: List[Segment], max_audio_length_ms: float = 90_000,
                 temperature: float = 0.7, topk: int = 30, stream: bool = False, session: Optional[Conversation] = None,
                 speed=None, watermark=None) -> torch.Tensor:
        """reference: generator.py:212-300.  ``session``: ``context`` lists only the segments that are NEW since the session's last turn
        (``open_session``).  ``speed`` (None: the calls above exactly): a speech-rate factor in 0.5 .. 2.0 -- the decoded clip goes through a
        one-shot device time stretch (sesameai/stretch.py); the pitch stays.  ``watermark`` (None: the calls above exactly): True, "device"
        or a five-byte key -- the clip then carries the device watermark (sesameai/watermarking.py), embedded after the stretch."""
        (how_fast,) = self._speeds(speed, 1)
        if (key := self._mark_key(watermark)) is not None:
            audio = self.generate(text, speaker, context, max_audio_length_ms, temperature, topk, stream=stream, session=session,
                                  **({} if speed is None else {"speed": speed}))
            return self._mark_clip(audio, key)
        if stream:
            chunks = list(self.generate_stream(text, speaker, context, max_audio_length_ms, temperature, topk, session=session))
            audio = torch.cat(chunks) if chunks else torch.tensor([])
            return audio if how_fast is None else self._stretch_clip(audio, how_fast)
        max_generation_len = int(max_audio_length_ms / FRAME_MS)
        tokens, mask = self._build_prompt(text, speaker, context)
        frames = self.generate_codes(tokens, mask, max_generation_len, temperature, topk, session=session)
        if frames.shape[0] == 0:
            return torch.tensor([])
        audio = self._decode_frames(frames)
        return audio if how_fast is None else self._stretch_clip(audio, how_fast)


def _wav_float32_header(sample_rate: int, data_bytes: int) -> bytes:
    """44-byte RIFF header of a mono 32-bit IEEE-float WAV (format tag 3) -- what ``torchaudio.save(file, audio.unsqueeze(0), sr)``
    writes for a float32 tensor (reference: generator.py:327); torchaudio is not a dependency here."""
    return (b"RIFF" + struct.pack("<I", 36 + data_bytes) + b"WAVE"
            + b"fmt " + struct.pack("<IHHIIHH", 16, 3, 1, sample_rate, sample_rate * 4, 4, 32)
            + b"data" + struct.pack("<I", data_bytes))


def _float32_bytes(audio: torch.Tensor) -> bytes:
    return audio.detach().to(torch.float32).reshape(-1).cpu().contiguous().numpy().astype("<f4", copy=False).tobytes()


def save_wav_float32(filename: str, audio: torch.Tensor, sample_rate: int) -> None:
    """(n,) float samples -> mono float32 WAV in one go."""
    pcm = _float32_bytes(audio)
    with open(filename, "wb") as f:
        f.write(_wav_float32_header(sample_rate, len(pcm)) + pcm)


class AudioStreamWriter:
    """The reference's streaming file writer (sesameai/generator.py:303-327: ``add_chunk`` from the generation loop, one
    ``write_file`` at the end) with a bounded footprint: every chunk is appended to the OPEN file as it arrives and
    ``write_file`` only patches the two RIFF size fields and closes -- a 90 s utterance never sits in memory as a list of
    tensors, and a run that dies half-way leaves the audio produced so far on disk.  No chunk, no file (the reference
    returns before ``torchaudio.save`` then).  ``add_chunk`` may be called from another thread than ``write_file``.

    Until ``write_file`` the header carries the streaming placeholder 0xFFFFFFFF in both size fields ("length unknown": players
    read to the end of the file), so a writer that is abandoned -- dropped, garbage-collected, the process killed -- leaves a WAV
    that still plays; ``close()`` / ``with`` / ``__del__`` finalise it like ``write_file``.  The reference's public ``audio_chunks``
    list is kept as an attribute for callers that look at it, but stays EMPTY here (the chunks are in the file); ``chunks_written``
    counts them."""

    _UNKNOWN = 0xFFFFFFFF

    def __init__(self, filename, sample_rate):
        self.filename = filename
        self.sample_rate = sample_rate
        self.lock = threading.Lock()
        self.audio_chunks: List[torch.Tensor] = []       # reference attribute; not filled (see the class docstring)
        self.chunks_written = 0
        self._file = None
        self._data_bytes = 0

    def add_chunk(self, chunk):
        pcm = _float32_bytes(chunk)                      # (the device -> host copy happens outside the lock)
        with self.lock:
            if self._file is None:
                self._file = open(self.filename, "wb")
                hdr = bytearray(_wav_float32_header(self.sample_rate, 0))
                hdr[4:8] = struct.pack("<I", self._UNKNOWN); hdr[40:44] = struct.pack("<I", self._UNKNOWN)
                self._file.write(bytes(hdr))
            self._file.write(pcm)
            self._data_bytes += len(pcm)
            self.chunks_written += 1

    def write_file(self):
        with self.lock:
            if self._file is None:
                return
            f, self._file = self._file, None
            f.seek(4); f.write(struct.pack("<I", 36 + self._data_bytes))
            f.seek(40); f.write(struct.pack("<I", self._data_bytes))
            f.close()

    close = write_file

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.write_file()
        return False

    def __del__(self):
        try:
            self.write_file()
        except Exception:
            pass


class _ChunkPlayer:
    """Real-time playback of streamed chunks in arrival order (reference: the ``audio_player`` thread of
    generate_streaming_audio, generator.py:384-404) through the optional ``sounddevice`` package.  One worker drains a queue
    until it meets the end marker ``close()`` posts, so nothing polls with time-outs and every queued chunk is played before
    ``close()`` returns.  Raises ImportError at construction when ``sounddevice`` is missing."""

    _END = object()

    def __init__(self, sample_rate: int):
        import sounddevice
        self._sd, self._rate = sounddevice, sample_rate
        self._chunks: "queue.Queue" = queue.Queue()
        self._worker = threading.Thread(target=self._drain, name="csm-chunk-player")
        self._worker.start()

    def _drain(self) -> None:
        for chunk in iter(self._chunks.get, self._END):
            self._sd.play(chunk.detach().to(torch.float32).cpu().numpy(), self._rate)
            self._sd.wait()

    def submit(self, chunk: torch.Tensor) -> None:
        self._chunks.put(chunk)

    def close(self) -> None:
        self._chunks.put(self._END)
        self._worker.join()


def generate_streaming_audio(generator: "Generator", text, speaker: int, context: List[Segment], output_file: str,
                             max_audio_length_ms: float = 90_000, temperature: float = 0.7, topk: int = 30,
                             play_audio: bool = False):
    """reference: sesameai/generator.py:349-434 (same arguments, same console messages): ``generate_stream`` with every chunk
    appended to ``output_file`` as it is produced and, with ``play_audio``, played as it arrives.  Without ``sounddevice``
    playback is switched off with the reference's message and the file is still written."""
    sinks: List[Callable[[torch.Tensor], None]] = []
    writer = AudioStreamWriter(output_file, generator.sample_rate)
    sinks.append(writer.add_chunk)
    player: Optional[_ChunkPlayer] = None
    if play_audio:
        try:
            player = _ChunkPlayer(generator.sample_rate)
            sinks.append(player.submit)
        except ImportError:
            print("sounddevice library not found. Install with 'pip install sounddevice' to enable real-time playback.")

    print("Generating audio in streaming mode...")
    t0 = time.time()
    try:
        stream = generator.generate_stream(text=text, speaker=speaker, context=context, max_audio_length_ms=max_audio_length_ms,
                                           temperature=temperature, topk=topk)
        for n, chunk in enumerate(stream, start=1):
            for sink in sinks:
                sink(chunk)
            print(f"Generated chunk {n}")
    finally:
        writer.write_file()                              # whatever was generated is a valid WAV, also after an error
        if player is not None:
            player.close()
    print(f"Audio generation completed in {time.time() - t0:.2f} seconds")


def load_csm_1b(device: str = "cuda", model_path: Optional[str] = None, mimi_path: Optional[str] = None,
                max_batch_size: int = 1, synthetic: Optional[bool] = None) -> Generator:
    """reference: sesameai/generator.py:330-346.  The reference downloads ``sesame/csm-1b`` and the Mimi
    checkpoint from the hub; there is no network here, so ``model_path`` / ``mimi_path`` (or $CSM_MODEL_PATH /
    $CSM_MIMI_PATH) must name local files.  Seeded random weights of the true shapes (benchmarks, tests)
    are used ONLY when asked for -- ``synthetic=True`` or $CSM_SYNTHETIC=1 -- never as a silent fallback:
    a TTS service that writes noise and exits 0 is worse than one that refuses to start."""
    model_path = model_path or os.environ.get("CSM_MODEL_PATH")
    mimi_path = mimi_path or os.environ.get("CSM_MIMI_PATH")
    if synthetic is None:
        synthetic = os.environ.get("CSM_SYNTHETIC") == "1"
    if not synthetic and not (model_path and mimi_path):
        raise FileNotFoundError("load_csm_1b: set CSM_MODEL_PATH (sesame/csm-1b model.safetensors) and CSM_MIMI_PATH (moshi "
                                "tokenizer safetensors) or pass model_path= / mimi_path=; for seeded random weights "
                                "(benchmarks, tests) pass synthetic=True or set CSM_SYNTHETIC=1")
    model = Model.from_pretrained(model_path, device=device) if model_path else Model(csm_1b_args(), None, device=device)
    from .mimi import MimiCodec
    mimi = MimiCodec.from_pretrained(mimi_path, device=device)
    gen = Generator(model, audio_tokenizer=mimi, max_batch_size=max_batch_size)
    if os.environ.get("CSM_NO_WARMUP") != "1":
        gen.warm_up()
    return gen
