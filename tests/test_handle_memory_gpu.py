"""Who owns a CSM handle's device memory (sesameai-tts_amd/csrc/dev_pool.h, csm_create / csm_destroy in csm_engine.hip): a refused
csm_create gives back everything it had allocated and leaves the process fit for the next create; create / destroy cycles that bring the
lazily made workspaces into play (the refill buffers, the group tables) return to the same free memory and the same frames.

64 MiB is the margin tools/leak_check.py allows for the allocator's granularity."""
import gc

import pytest
import torch

pytestmark = pytest.mark.gpu
MARGIN = 64 << 20


def _prompt(seed, S=4):
    g = torch.Generator().manual_seed(seed)
    tok = torch.zeros(S, 33, dtype=torch.long); msk = torch.zeros(S, 33, dtype=torch.bool)
    tok[:2, 32] = torch.randint(0, 1000, (2,), generator=g); msk[:2, 32] = True
    tok[2:, :32] = torch.randint(0, 2048, (S - 2, 32), generator=g); msk[2:, :32] = True
    return tok, msk


def _free_bytes():
    gc.collect()                        # (a caught exception's traceback keeps the frames it passed through, and their models, until collected)
    torch.cuda.synchronize(); torch.cuda.empty_cache()
    return torch.cuda.mem_get_info()[0]


def test_a_refused_create_gives_everything_back_and_the_next_create_is_unharmed():
    """A frame history of 2^31 x 256 x 32 x 4 bytes (about 70 TB) is refused by the runtime on the host side, after the caches and
    workspaces in front of it (about 67 MB, the two backbone caches 33.5 MB each) were allocated: nothing of them may stay behind, eight
    times over, and an ordinary handle made afterwards in the same process must produce the bits it produced before."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from sesameai.models import Model, csm_tiny_args, synthetic_state_dict
    sd = synthetic_state_dict(csm_tiny_args(), seed=1234)
    tok, msk = _prompt(8)

    def ordinary_frames():
        m = Model(csm_tiny_args(), sd, max_frames=32, max_prefill_rows=64)
        m.setup_caches(1)
        m.seed(7)
        m.prefill_prompt(tok.unsqueeze(0), msk.unsqueeze(0))
        m.depth(1, 0.9, 50, commit=True)
        for _ in range(3):
            m.step(1, 0.9, 50)
        return m.read_frames(1)[0].clone()

    want = ordinary_frames()
    assert want.shape == (4, 1, 32)
    free0 = _free_bytes()
    for i in range(8):
        m = Model(csm_tiny_args(), sd, max_frames=2**31 - 1)
        with pytest.raises(RuntimeError) as err:
            m.setup_caches(256)
        msg = str(err.value)
        del err                         # (its traceback holds setup_caches' frame, and with it the model and its weights)
        assert "history" in msg, f"create {i}: the error does not name the allocation that failed: {msg}"
        assert not m.caches_are_enabled()
        del m
        print(f"refused create {i + 1}: {msg}; {_free_bytes() >> 20} MiB free")
    free1 = _free_bytes()
    print(f"free device memory: {free0 >> 20} MiB before, {free1 >> 20} MiB after 8 refused creates")
    assert abs(free0 - free1) < MARGIN, f"8 refused creates left {(free0 - free1) >> 20} MiB of device memory behind"
    assert torch.equal(ordinary_frames(), want), "a handle made after the refused creates does not produce the frames it produced before them"


def test_create_destroy_cycles_with_the_lazy_workspaces_in_play():
    """Six cycles, bf16 and fp8 in turn: re-create the handle twice, a single refill and a group refill beside the loop (each makes its
    workspace at first use) with a frame step after each, destroy.  Two additions make the listed calls well defined: the refills need a
    handle of max batch 4 (one of max batch 2 has no matrix-core decode path and refuses them), so after setup_caches(4) and
    setup_caches(2) the handle is made once more at 4; and every slot gets a prompt and its frame 0 first, because the row of a slot that
    never held an utterance is computed from token memory nothing has written, which no cycle can be expected to repeat."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from sesameai.models import Model, csm_tiny_args, synthetic_state_dict
    sd = synthetic_state_dict(csm_tiny_args(), seed=1234)
    prompts = [_prompt(s) for s in (21, 22, 23)]
    first = [_prompt(s) for s in (31, 32, 33, 34)]
    tok4, msk4 = torch.stack([t for t, _ in first]), torch.stack([k for _, k in first])
    frames, free = [], []
    for cycle in range(6):
        m = Model(csm_tiny_args(), sd, max_frames=32, max_prefill_rows=64, weights_dtype="fp8" if cycle % 2 else "bf16")
        m.setup_caches(4)
        m.setup_caches(2)
        m.setup_caches(4)
        assert m.supports_refill_beside_the_loop(4)
        m.seed(7)
        m.prefill_prompt(tok4, msk4)
        m.depth(4, 0.9, 50, commit=True)
        m.refill_begin(1, *prompts[0])
        while not m.refill_advance(1):
            pass
        m.step(4, 0.9, 50)
        m.refill_group_begin([0, 3], prompts[1:])
        while not m.refill_group_advance(1):
            pass
        m.step(4, 0.9, 50)
        frames.append(m.read_frames(4)[0].clone())
        del m
        free.append(_free_bytes())
    print("free device memory after each cycle, MiB:", [f >> 20 for f in free])
    assert frames[0].shape == (3, 4, 32)
    for a, b in ((4, 0), (5, 1)):
        print(f"cycle {a + 1} vs cycle {b + 1}: (frame, slot) rows that differ:", (frames[a] != frames[b]).any(dim=2).nonzero().tolist())
    for cycle in range(1, 6):
        assert abs(free[cycle] - free[0]) < MARGIN, f"cycle {cycle + 1}: {(free[0] - free[cycle]) >> 20} MiB less free than after cycle 1"
    assert torch.equal(frames[4], frames[0]), "bf16: cycle 5 does not produce the frames of cycle 1"
    assert torch.equal(frames[5], frames[1]), "fp8: cycle 6 does not produce the frames of cycle 2"
