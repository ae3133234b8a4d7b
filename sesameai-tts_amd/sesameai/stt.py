"""A thin adapter from the device's log-mel features (sesameai/mel.py) to a Whisper-family recogniser that the USER has loaded, from a local
path, with transformers.  Nothing is downloaded and nothing of transformers is imported at module level: the model and the tokenizer are the
caller's objects, and the adapter only calls them.  With ``encoder=`` the model's encoder -- the recogniser's hot path -- runs in this
library (sesameai/whisper_enc.py) and ``generate`` gets its output; the decoder and the tokenizer stay the caller's."""
from __future__ import annotations

from typing import List, Optional, Sequence, Tuple

import torch


class WhisperSTT:
    """``WhisperSTT(model, processor_or_tokenizer, dtype=None, encoder=None)(features, n_frames) -> str``: what ``ReplyOnPause(stt=)`` takes.
    model: a transformers Whisper model for conditional generation (distil-whisper and every Whisper size take the same input);
    processor_or_tokenizer: anything with ``batch_decode(ids, skip_special_tokens=True)``; dtype: the model's input dtype (None: its own).
    encoder: None (the model's own encoder, through ``generate(input_features=)``), ``"device"`` (a ``WhisperEncoder.from_model(model)``) or
    a ``WhisperEncoder``: its output goes to ``generate(encoder_outputs=)``; max_batch: the turns one ``transcribe_many`` encode takes
    when ``"device"`` builds the encoder.  ``generate_kwargs`` go to ``model.generate``."""

    def __init__(self, model, processor_or_tokenizer, dtype: Optional[torch.dtype] = None, encoder=None, max_batch: int = 1, **generate_kwargs):
        self.model, self.decoder, self.generate_kwargs = model, processor_or_tokenizer, generate_kwargs
        self.dtype = dtype if dtype is not None else getattr(model, "dtype", torch.float32)
        if isinstance(encoder, str):
            if encoder != "device":
                raise ValueError('encoder must be None, "device" or a WhisperEncoder')
            from .whisper_enc import WhisperEncoder
            encoder = WhisperEncoder.from_model(model, max_batch=max_batch)
        self.encoder = encoder

    @torch.inference_mode()
    def __call__(self, features: torch.Tensor, n_frames: int = 0) -> str:
        if self.encoder is not None:
            return self.transcribe_many([(features, n_frames)])[0]
        assert features.dim() == 2 and features.shape[1] == 3000, "features must be (n_mels, 3000)"
        ids = self.model.generate(input_features=features[None].to(self.dtype), **self.generate_kwargs)
        return self.decoder.batch_decode(ids, skip_special_tokens=True)[0].strip()

    @torch.inference_mode()
    def transcribe_many(self, turns: Sequence[Tuple[torch.Tensor, int]]) -> List[str]:
        """turns: [(features (n_mels, 2 n_ctx), n_frames)] -> their texts.  With an encoder, up to its ``max_batch`` turns share one encode
        and one ``generate``; without one, each turn is a call of its own."""
        if self.encoder is None:
            return [self(f, n) for f, n in turns]
        from transformers.modeling_outputs import BaseModelOutput      # (a bare tuple is refused by generate)
        out: List[str] = []
        step = max(1, int(getattr(self.encoder, "max_batch", 1)))
        for i in range(0, len(turns), step):
            feats = torch.stack([f for f, _ in turns[i:i + step]])
            assert feats.dim() == 3, "features must be (n_mels, 2 n_ctx)"
            h = self.encoder.encode(feats)
            model_dtype = getattr(self.model, "dtype", None) or self.dtype
            ids = self.model.generate(encoder_outputs=BaseModelOutput(last_hidden_state=h.to(model_dtype)), **self.generate_kwargs)
            out += [t.strip() for t in self.decoder.batch_decode(ids, skip_special_tokens=True)]
        return out
