"""Preconditions of the encode-stream tests (tests/test_mimi_enc_stream_gpu.py), on the CPU oracle alone (oracle/mimi_ref.py): the GPU tests
compare a stream's codes with the whole-clip encode, and these show that they could not pass by accident -- every piece of state a stream
carries across a call boundary, every edge mode and the RoPE position move codes on this codec, these weights and this kind of clip.

The streaming encoder below restates ``M.encode_latent`` chunk by chunk with explicit left context per convolution, so that each piece of
state can be dropped on its own.  Its faultless form is checked against ``M.encode`` first; every fault is then compared with the faultless
stream (same chunking, so the same torch convolution calls: a difference is the fault's, not a rounding change between two call shapes).
Only "at least one frame of every later chunk" and "the last frame" are asserted, never a list of frames."""
import torch
import torch.nn.functional as F

from oracle import mimi_ref as M

HOP = 1920
CUTS = [0, 2, 5, 6, 12]                # in frames: chunks of 2, 3, 1 and 6 frames
TAILS = [1, 777, 960, 961]


def _clip(seed, n):
    return torch.randn(n, generator=torch.Generator().manual_seed(seed)) * 0.3


def _model():
    s = M.mimi_tiny()
    return s, M.make_weights(s, seed=4321, encoder=True)


def _conv_ctx(x, hist, w, b, stride=1, pad_mode="constant"):
    """causal Conv1d over one chunk x (1,C,n) with its left context hist (1,C,k-stride); right padding as the oracle's
    ``_strided_causal_conv`` gives the END of a clip: up to ceil(n / stride) outputs"""
    k = w.shape[-1]
    assert hist.shape[-1] == k - stride
    n_out = -(-x.shape[-1] // stride)
    xx = torch.cat([hist, x], dim=-1)
    extra = (n_out - 1) * stride + k - xx.shape[-1]
    if extra > 0:
        xx = F.pad(xx, (0, extra), mode=pad_mode)
    return F.conv1d(xx, w, b, stride=stride)


@torch.inference_mode()
def stream_encode(s, w, wav, cuts, kv=True, seanet=True, down_hist=True, first_replicate=True, context=None, rope_mod=None):
    """wav (n,) -> codes (32, T), encoded chunk by chunk at the sample offsets ``cuts`` (the last: n).  Faults: kv=False forgets the
    transformer's keys and values at every cut (positions go on); seanet=False zeroes every convolution's left context at every cut;
    down_hist=False lets the downsample replicate its chunk's first token at every cut instead of reading the two tokens before it;
    first_replicate=False gives the downsample zeros, not the first token, in front of the stream."""
    hist = {}                           # name -> the last k - stride input columns of that convolution
    tok_in = []                         # the transformer's inputs so far (1, t, d)
    out, off = [], 0

    def conv(name, x, wn, stride=1, act=True):
        xin = F.elu(x) if act else x
        k = w[wn + ".weight"].shape[-1]
        h = hist.get(name)
        if h is None or not seanet:
            h = torch.zeros(1, xin.shape[1], k - stride)
        y = _conv_ctx(xin, h, w[wn + ".weight"], w.get(wn + ".bias"), stride)
        if k - stride:
            hist[name] = torch.cat([h, xin], dim=-1)[..., -(k - stride):]
        return y

    for a, b in zip(cuts[:-1], cuts[1:]):
        x = conv("in", wav[a:b].view(1, 1, -1), "enc.conv_in", act=False)
        for j, r in enumerate(reversed(s.ratios)):
            y = conv(f"r1.{j}", x, f"enc.down.{j}.res.conv1")
            y = conv(f"r2.{j}", y, f"enc.down.{j}.res.conv2")
            x = x + y
            x = conv(f"dn.{j}", x, f"enc.down.{j}.conv", stride=r)
        x = conv("out", x, "enc.conv_out").transpose(1, 2)            # (1, L, d)
        L = x.shape[1]
        tok_in.append(x)
        if kv:      # causal: the chunk's rows of the transformer over everything so far are the rows a K/V cache gives
            z = M.transformer(s, w, torch.cat(tok_in, dim=1), prefix="enc_transformer", context=context, rope_mod=rope_mod)[:, -L:]
        else:
            z = M.transformer(s, w, x, offset=off, prefix="enc_transformer", context=context, rope_mod=rope_mod)
        z = z.transpose(1, 2)
        if off == 0 or not down_hist:
            h = z[..., :1].expand(-1, -1, 2) if (first_replicate or off != 0) else torch.zeros(1, z.shape[1], 2)
        else:
            h = hist["down"]
        hist["down"] = torch.cat([h, z], dim=-1)[..., -2:]
        out.append(_conv_ctx(z, h, w["downsample.conv.weight"], None, 2, pad_mode="replicate"))
        off += L
    return M.quantize(s, w, torch.cat(out, dim=-1))[0]


def _changed(a, b):
    return (a != b).any(dim=0)


def _every_later_chunk_changes(got, want, what):
    ch = _changed(got, want)
    print(f"{what}: frames changed {ch.nonzero().flatten().tolist()}")
    assert not ch[:CUTS[1]].any(), f"{what}: the first chunk moved"
    for a, b in zip(CUTS[1:-1], CUTS[2:]):
        assert ch[a:b].any(), f"{what}: no frame of chunk [{a}, {b}) changes"


def test_a_prefix_of_the_clip_encodes_to_a_prefix_of_the_codes():
    s, w = _model()
    x = _clip(301, 12 * HOP)
    whole = M.encode(s, w, x.view(1, 1, -1))[0]
    assert whole.shape == (32, 12)
    for k in (1, 2, 5, 12):
        assert torch.equal(M.encode(s, w, x[:k * HOP].view(1, 1, -1))[0], whole[:, :k]), f"the first {k} frames depend on what follows"


def test_every_piece_of_carried_state_moves_codes():
    s, w = _model()
    x = _clip(301, 12 * HOP)
    whole = M.encode(s, w, x.view(1, 1, -1))[0]
    cuts = [c * HOP for c in CUTS]
    good = stream_encode(s, w, x, cuts)
    same = (~_changed(good, whole)).float().mean().item()
    print(f"the faultless stream against the whole-clip oracle: {same:.3f} of the frames identical")
    assert same >= 0.9, "the streaming restatement is not the oracle's encode"
    # a chunk encoded alone: all state lost at once
    alone = torch.cat([M.encode(s, w, x[a:b].view(1, 1, -1))[0] for a, b in zip(cuts[:-1], cuts[1:])], dim=1)
    _every_later_chunk_changes(alone, whole, "every chunk encoded alone")
    _every_later_chunk_changes(stream_encode(s, w, x, cuts, kv=False), good, "K/V lost at each cut")
    _every_later_chunk_changes(stream_encode(s, w, x, cuts, seanet=False), good, "SEANet history lost at each cut")
    _every_later_chunk_changes(stream_encode(s, w, x, cuts, down_hist=False), good, "downsample replicates at each cut")
    ch = _changed(stream_encode(s, w, x, cuts, first_replicate=False), good)
    print(f"zero left edge of the downsample at the start: frames changed {ch.nonzero().flatten().tolist()}")
    assert ch[0] and not ch[1:].any()


def test_rope_position_and_window_length_move_codes():
    s, w = _model()
    x = _clip(301, 12 * HOP).view(1, 1, -1)
    whole = M.encode(s, w, x)[0]
    for kw in ({"rope_mod": 12}, {"rope_mod": 14}, {"context": 5}, {"context": 7}):
        ch = _changed(M.encode(s, w, x, **kw)[0], whole)
        print(f"{kw}: frames changed {ch.nonzero().flatten().tolist()}")
        assert ch.any(), f"{kw} leaves every code in place"


def test_the_tail_rule_is_not_zero_padding_of_the_input():
    s, w = _model()
    for r in TAILS:
        x = _clip(310 + r, 2 * HOP + r)
        want = M.encode(s, w, x.view(1, 1, -1))[0]
        padded = M.encode(s, w, F.pad(x, (0, HOP - r)).view(1, 1, -1))[0]
        assert want.shape == padded.shape == (32, 3)
        n = int((want[:, -1] != padded[:, -1]).sum())
        print(f"r = {r}: zero-padding the input to the frame boundary changes {n} of 32 codes of the last frame")
        assert torch.equal(want[:, :-1], padded[:, :-1]), "padding behind the clip moved an earlier frame"
        assert n > 0, f"r = {r}: the last frame does not tell the tail rule from zero padding"
        # ... and the faultless stream takes the tail as the whole-clip encode does, as its last chunk's rows alone
        got = stream_encode(s, w, x, [0, HOP, 2 * HOP + r])
        assert torch.equal(got[:, -1], want[:, -1]), f"r = {r}: the streamed tail differs from the whole-clip tail"
