"""A thin adapter from the device's log-mel features (sesameai/mel.py) to a Whisper-family recogniser that the USER has loaded, from a local
path, with transformers.  Nothing is downloaded and nothing of transformers is imported here: the model and the tokenizer are the caller's
objects, and the adapter only calls them."""
from __future__ import annotations

from typing import Optional

import torch


class WhisperSTT:
    """``WhisperSTT(model, processor_or_tokenizer, dtype=None)(features, n_frames) -> str``: what ``ReplyOnPause(stt=)`` takes.
    model: a transformers Whisper model for conditional generation (distil-whisper and every Whisper size take the same input);
    processor_or_tokenizer: anything with ``batch_decode(ids, skip_special_tokens=True)``; dtype: the model's input dtype (None: its own).
    ``generate_kwargs`` go to ``model.generate``."""

    def __init__(self, model, processor_or_tokenizer, dtype: Optional[torch.dtype] = None, **generate_kwargs):
        self.model, self.decoder, self.generate_kwargs = model, processor_or_tokenizer, generate_kwargs
        self.dtype = dtype if dtype is not None else getattr(model, "dtype", torch.float32)

    @torch.inference_mode()
    def __call__(self, features: torch.Tensor, n_frames: int = 0) -> str:
        assert features.dim() == 2 and features.shape[1] == 3000, "features must be (n_mels, 3000)"
        ids = self.model.generate(input_features=features[None].to(self.dtype), **self.generate_kwargs)
        return self.decoder.batch_decode(ids, skip_special_tokens=True)[0].strip()
