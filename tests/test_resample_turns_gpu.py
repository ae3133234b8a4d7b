"""The resampler pool where audio enters and leaves (tiny codec, tiny model): a 48 kHz int16 and a 16 kHz fp32 microphone through
``TurnStreams``, clips at their own rates through ``encode`` / ``encode_many``, and ``generate_many_stream`` handing out 48 kHz.  Everything is
bit for bit what the whole-clip calls give: the resampler's streamed == one-shot rule under the encode pool's own."""
import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def codec():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from sesameai.mimi import MimiCodec, mimi_tiny_args, synthetic_state_dict
    return MimiCodec(mimi_tiny_args(), synthetic_state_dict(mimi_tiny_args(), seed=4321), max_frames=64)


def _turn(rate, seconds, seed, int16):
    g = torch.Generator().manual_seed(seed)
    x = 0.3 * torch.randn(int(rate * seconds) + 123, generator=g)
    return (x.clamp(-1, 1) * 32767).round().to(torch.int16) if int16 else x


@pytest.mark.parametrize("rate, int16", [(48000, True), (16000, False)])
def test_a_turn_at_the_microphones_rate_is_encode_of_its_resampled_whole(codec, rate, int16):
    from sesameai.generator import Generator
    from sesameai.resample import resample
    gen = Generator.__new__(Generator)
    gen._audio_tokenizer, gen.sample_rate, gen.device = codec, codec.sample_rate, codec.device
    ts = gen.open_turn_streams(3, chunk_frames=4, sample_rate=rate)
    assert ts.resampler is not None and (ts.resampler.src_rate, ts.resampler.dst_rate) == (rate, 24000)
    a, b = _turn(rate, 0.5, 1, int16), _turn(rate, 0.3, 2, int16)
    cuts_a, cuts_b = [0, 1000, 1037, 6037, 6038, a.shape[0]], [0, 5, 4000, 4001, 4001, b.shape[0]]
    for k in range(5):                                                   # two microphones, uneven feeds, a pump after every round
        ts.feed(2, a[cuts_a[k]:cuts_a[k + 1]].cuda()); ts.feed(0, b[cuts_b[k]:cuts_b[k + 1]])
        ts.pump()
    seg_b = ts.finish(0, 1, [7])
    seg_a = ts.finish(2, 1, [8, 9])
    for seg, x in ((seg_a, a), (seg_b, b)):
        (whole,) = resample([x.cuda()], rate, 24000)
        want = codec.encode(whole[None, None])[0]
        assert seg.audio_codes.shape == want.shape and torch.equal(seg.audio_codes, want)
        assert torch.equal(codec.encode(x.cuda()[None, None], sample_rate=rate)[0], want), "encode(sample_rate=) is encode of the resampled clip"
    # the streams start their next turns from scratch
    ts.feed(2, b.cuda())
    assert torch.equal(ts.finish(2, 1, [1]).audio_codes, seg_b.audio_codes)


def test_encode_many_takes_every_clip_at_its_own_rate(codec):
    clips = [_turn(48000, 0.25, 3, True), _turn(24000, 0.2, 4, False), _turn(16000, 0.3, 5, False), _turn(48000, 0.1, 6, False)]
    rates = [48000, None, 16000, 48000]
    got = codec.encode_many([c.cuda() for c in clips], sample_rates=rates)
    for c, r, g in zip(clips, rates, got):
        want = codec.encode(c.cuda()[None, None], **({} if r is None else {"sample_rate": r}))[0]
        assert g.shape == want.shape and torch.equal(g, want), f"clip at {r}"
    plain = codec.encode_many([clips[1].cuda()])
    assert torch.equal(plain[0], got[1])
    one_rate = codec.encode_many([clips[0].cuda(), clips[3].cuda()], sample_rates=48000)
    assert torch.equal(one_rate[0], got[0]) and torch.equal(one_rate[1], got[3])


def test_segments_carry_their_rate_into_the_prompt(codec):
    from sesameai.generator import Generator, Segment
    gen = Generator.__new__(Generator)
    gen._audio_tokenizer, gen.sample_rate, gen.device, gen._text_tokenizer = codec, codec.sample_rate, codec.device, None
    a, b = _turn(48000, 0.25, 3, True).cuda(), _turn(24000, 0.2, 4, False).cuda()
    ctx = [Segment(1, [5], audio=a, sample_rate=48000), Segment(0, [6], audio=b)]
    want = [Segment(1, [5], audio_codes=codec.encode(a[None, None], sample_rate=48000)[0]), Segment(0, [6], audio_codes=codec.encode(b[None, None])[0])]
    t, m = gen._build_prompt([1, 2], 0, ctx)                             # two clips: the ragged encode
    t2, m2 = gen._build_prompt([1, 2], 0, want)
    assert torch.equal(t, t2) and torch.equal(m, m2)
    t1, _ = gen._build_prompt([1, 2], 0, ctx[:1])                        # one clip: the single encode
    t3, _ = gen._build_prompt([1, 2], 0, want[:1])
    assert torch.equal(t1, t3)


@pytest.mark.parametrize("out_dtype", [None, torch.int16])
def test_generate_many_stream_hands_out_48_khz(codec, out_dtype):
    """Greedy (top-k 1), so the plain run and the 48 kHz run generate the same frames.  A request of 10 or 20 frames may close with a chunk
    that is empty at 24 kHz: it still carries the filter's tail (tests/test_resample_host_logic.py forces that case).  The request limited to
    0 frames takes the path of a first frame that is EOS (an empty utterance, sesameai/live_batch.py) and yields zero samples."""
    from sesameai.generator import Generator, Segment
    from sesameai.models import Model, csm_tiny_args
    from sesameai.resample import resample
    model = Model(csm_tiny_args(), None, max_frames=64, max_prefill_rows=128)
    gen = Generator(model, audio_tokenizer=codec, max_batch_size=3)
    gen.refill_row_layers = 10
    g = torch.Generator().manual_seed(21)
    lens = [27, 3, 10, 0, 14, 20, 1]
    texts = [torch.randint(0, 1000, (4 + i % 5,), generator=g).tolist() for i in range(len(lens))]
    ctxs = [[Segment(speaker=1, text=torch.randint(0, 1000, (3,), generator=g).tolist(), audio_codes=torch.randint(0, 2048, (32, 2 + i % 4), generator=g))]
            for i in range(len(lens))]
    ms = [n * 80 for n in lens]

    def run(**kw):
        got = {i: [] for i in range(len(lens))}
        for i, pcm, frames, last in gen.generate_many_stream(texts, [1] * len(lens), ctxs, max_audio_length_ms=ms, temperature=0.9, topk=1, **kw):
            got[i].append((pcm, frames, last))
        return got
    plain = run()
    kw = {"out_sample_rate": 48000, **({} if out_dtype is None else {"out_dtype": out_dtype})}
    fast = run(**kw)
    for i, n in enumerate(lens):
        a, b = plain[i], fast[i]
        assert [c[2] for c in b] == [False] * (len(b) - 1) + [True]
        assert torch.equal(torch.cat([c[1] for c in a]), torch.cat([c[1] for c in b])) and sum(c[1].shape[0] for c in b) == n
        pcm24 = torch.cat([c[0] for c in a])
        pcm48 = torch.cat([c[0] for c in b])
        assert pcm48.dtype == (out_dtype or torch.float32)
        if n == 0:
            assert pcm48.numel() == 0 and len(b) == 1
            continue
        (want,) = resample([pcm24], 24000, 48000, out_dtype=out_dtype or torch.float32)
        assert pcm48.shape == want.shape == (2 * 1920 * n,) and torch.equal(pcm48, want), f"request {i} ({n} frames)"
        if b[-1][1].shape[0] == 0:
            assert b[-1][0].numel() > 0, "a closing chunk that is empty at 24 kHz carries the tail"
        assert sum(c[0].numel() for c in b[:-1]) < 2 * sum(c[0].numel() for c in a[:-1]) or len(b) == 1, "the look-ahead is held back until the close"
    again = run()
    assert all(torch.equal(torch.cat([c[0] for c in again[i]]), torch.cat([c[0] for c in plain[i]])) for i in plain), "the plain path is what it was"
