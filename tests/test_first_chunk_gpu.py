"""``generate_many_stream(first_chunk_frames=k)`` end to end on the tiny model and the tiny codec (the set-up of
tests/test_mimi_streams_gpu.py::test_generate_many_stream_end_to_end_tiny): 12 requests with seeds of their own through a batch of 4, one
of them with limit 0.  With k in {1, 3}, on both refill policies, every request's frames are those of the run without the keyword (own
seeds: the draws do not depend on the block schedule), its chunks concatenated are bit for bit the codec's whole-clip decode of its
frames, and its first chunk has at least k frames."""
import pytest
import torch

pytestmark = pytest.mark.gpu
LENS = [27, 3, 10, 0, 14, 20, 1, 9, 11, 30, 5, 21]


@pytest.fixture(scope="module")
def setup():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from sesameai.generator import Generator, Segment
    from sesameai.mimi import MimiCodec, mimi_tiny_args, synthetic_state_dict
    from sesameai.models import Model, csm_tiny_args
    codec = MimiCodec(mimi_tiny_args(), synthetic_state_dict(mimi_tiny_args(), seed=4321), max_frames=64)
    model = Model(csm_tiny_args(), None, max_frames=64, max_prefill_rows=128)
    gen = Generator(model, audio_tokenizer=codec, max_batch_size=4)
    gen.refill_row_layers = 10
    g = torch.Generator().manual_seed(21)
    texts = [torch.randint(0, 1000, (4 + i % 5,), generator=g).tolist() for i in range(len(LENS))]
    ctxs = [[Segment(speaker=1, text=torch.randint(0, 1000, (3,), generator=g).tolist(), audio_codes=torch.randint(0, 2048, (32, 2 + i % 4), generator=g))]
            for i in range(len(LENS))]
    return gen, model, codec, texts, ctxs, {}


def _run(setup, beside, k):
    """{request: [(pcm, frames, last)]} of one run; the run without the keyword is made once per refill policy and shared."""
    gen, model, codec, texts, ctxs, cache = setup
    if (beside, k) in cache:
        return cache[(beside, k)]
    if beside:
        assert model.supports_refill_beside_the_loop(4)
    gen.refill_beside_the_loop = beside
    model.seed(5)
    got = {i: [] for i in range(len(LENS))}
    kw = {} if k is None else {"first_chunk_frames": k}
    for i, pcm, frames, last in gen.generate_many_stream(texts, [1] * len(LENS), ctxs, max_audio_length_ms=[n * 80 for n in LENS], temperature=0.9, topk=50,
                                                         seed=[1000 + i for i in range(len(LENS))], **kw):
        assert not (got[i] and got[i][-1][2]), f"request {i}: a chunk after its last one"
        assert pcm.dim() == 1 and pcm.dtype == torch.float32 and pcm.shape[0] == 1920 * frames.shape[0] and frames.shape[1:] == (32,)
        got[i].append((pcm.clone(), frames, last))
    cache[(beside, k)] = got
    return got


@pytest.mark.parametrize("beside", [True, False], ids=["refill_beside_the_loop", "refill_slot"])
@pytest.mark.parametrize("k", [1, 3])
def test_short_first_chunks_same_frames_same_audio(setup, beside, k):
    codec = setup[2]
    plain = _run(setup, beside, None)
    got = _run(setup, beside, k)
    early = 0
    for i, n in enumerate(LENS):
        assert [last for _, _, last in got[i]].count(True) == 1 and got[i][-1][2], f"request {i}: exactly one last chunk, at the end"
        frames = torch.cat([f for _, f, _ in got[i]])
        want = torch.cat([f for _, f, _ in plain[i]])
        assert want.shape[0] == n, "the random tiny model is not expected to sample an all-zero frame"
        assert torch.equal(frames, want), f"request {i}: with first_chunk_frames={k} its frames are not those of the run without"
        sizes = [f.shape[0] for _, f, _ in got[i]]
        assert min(k, n) <= sizes[0] <= 10 and all(sz == 10 for sz in sizes[1:-1]) and sizes[-1] <= 10, f"request {i}: chunks of {sizes} frames"
        early += sizes[0] < min(10, n)
        if n == 0:
            assert len(got[i]) == 1 and got[i][0][0].numel() == 0
            continue
        pcm = torch.cat([p for p, _, _ in got[i]])
        whole = codec.decode(frames.t().contiguous()[None].long())[0, 0]
        d = (pcm - whole).abs().max().item()
        print(f"k={k} request {i} ({n} frames, chunks {sizes}): max|d| vs whole-clip decode = {d:.3g}")
        assert torch.equal(pcm, whole), f"request {i}: chunks {sizes} vs the codec's whole-clip decode: max|d|={d:.3g}"
        assert torch.equal(pcm, torch.cat([p for p, _, _ in plain[i]])), f"request {i}: not the audio of the run without the keyword"
    assert early >= 4, "some first chunks should have left before a full chunk or the whole request was there"
