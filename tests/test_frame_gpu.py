"""Frame-level parity of the HIP path (through the reference-shaped surface
sesameai.models.Model / sesameai.generator.Generator) against the oracle and the committed
golden vectors.

Tolerances (bf16 path, as north_star asks "bit-exact for codebook indices under greedy"):
  * logits: max |HIP - oracle| <= 1x the oracle's own bf16-vs-fp32 gap (the rounding noise floor any bf16 implementation of this graph
    lives in) on the CSM-1B shapes -- at B = 1 and B = 4 the gap stored with the single-utterance goldens (measured: 0.4-0.7x), on the
    32-row batched paths the gap the oracle has ON THOSE 2,048 ROWS (oracle/make_golden.py cfg3gap / cfg5cgap; measured 0.81-0.82x) --
    and <= 1.25x on the tiny shapes, whose gap (0.018) is below one bf16 ulp of their logits (0.031 at |logit| >= 4; measured 1.07-1.13x = one ulp);
  * greedy indices, teacher-forced on the oracle trajectory: bit-exact wherever the oracle's own top-1/top-2 margin exceeds
    0.5x that noise floor on the CSM-1B shapes at B = 1 (round 4; 2x before, measured <= 0.42x), 1.0x on the batched paths (B >= 4: hundreds of
    decisions per frame, measured <= 0.84x) and 2x on the tiny shapes; the near-ties so
    excused are printed with their largest margin and their FRACTION is bounded (<= 8 % of the compared rows; measured 3-5 % with
    random weights, whose logits are nearly uniform).
"""
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(__file__), "golden")

# CSM-1B shapes: a greedy pick may differ from the oracle's only where the ORACLE's own top-1 / top-2 margin is at most NEAR_TIE x its
# bf16-vs-fp32 gap (0.112 on these shapes: 0.056; round 3 allowed 2 x although every excused row measured <= 0.047 -- VERDICT r3).
# The tiny shapes keep 2 x: their gap (0.018) is smaller than one bf16 ulp of their logits (0.031), so a 1-ulp move exceeds it.
NEAR_TIE = 0.5
BATCH32_TIE = 1.0        # near-tie bound of the BATCHED paths (B >= 4; 128..1,024 decisions per frame, 1,334-row prompts): the largest oracle margin at which a
                         # pick has been seen to differ is 0.094 = 0.84 x gap (config 5, B = 4 and 32, teacher-forced frame 0: two logits that moved 0.047 each,
                         # i.e. 0.42 x gap, towards each other) and 0.078 = 0.69 x gap (config 3 graph step); each logit may move by 1 x gap, so 2 x is the hard limit
_EXCUSED = []                                    # (what, margin, gap) of every excused row of the current test


def _excuse(margin, noise, what, tie=NEAR_TIE):
    _EXCUSED.append((what, float(margin), float(noise)))
    assert margin <= tie * noise, f"{what}: oracle margin {float(margin):.4f} > {tie} x gap {float(noise):.4f} -- not a near-tie"


@pytest.fixture(autouse=True)
def _report_excused_margins(request):
    _EXCUSED.clear()
    yield
    if _EXCUSED:
        worst = max(_EXCUSED, key=lambda e: e[1] / e[2])
        print(f"\n[parity] {request.node.name}: {len(_EXCUSED)} rows excused as near-ties, largest oracle margin {worst[1]:.4f} = "
              f"{worst[1] / worst[2]:.2f} x gap ({worst[0]})")


@pytest.fixture(scope="module")
def tiny():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from oracle import csm_ref as C
    from sesameai.models import Model, csm_tiny_args, synthetic_state_dict
    shape = C.csm_tiny()
    w = C.make_weights(shape, seed=1234)
    sd = synthetic_state_dict(csm_tiny_args(), seed=1234)
    assert all(torch.equal(w[k], sd[k]) for k in w), "product and oracle synthetic weights differ"
    m = Model(csm_tiny_args(), sd, max_frames=64, max_prefill_rows=256)
    m.setup_caches(4)
    return shape, w, m


def test_tiny_teacher_forced_vs_golden(tiny):
    shape, w, m = tiny
    gold = torch.load(os.path.join(GOLD, "tiny_frames.pt"))
    # step() runs a whole frame (backbone + depth + advance); for teacher forcing we need the
    # backbone step only, so drive the pieces: prefill/depth for frame 0, then generate_frame.
    tok, msk = gold["prompt_tokens"], gold["prompt_mask"]
    S = tok.shape[0]
    noise = float(gold["bf16_vs_fp32_gap"].max())
    m.reset_caches()
    m.prefill(tok.unsqueeze(0), msk.unsqueeze(0), torch.arange(S).unsqueeze(0))
    max_diff, mism = 0.0, []
    for f in range(gold["codes"].shape[0]):
        forced = gold["codes"][f].unsqueeze(0)
        out, logits = m.depth(1, 1.0, 1, forced=forced, want_logits=True, commit=False)
        d = (logits[:, 0].float().cpu() - gold["logits"][f].float()).abs().max().item()
        max_diff = max(max_diff, d)
        for cb in (out[0].cpu() != gold["codes"][f]).nonzero().flatten().tolist():
            mism.append((f, cb, float(gold["margin"][f, cb])))
        # next backbone row = the golden frame at position S+f (prefill API with S=1)
        row = torch.zeros(1, 1, 33, dtype=torch.long); row[0, 0, :32] = gold["codes"][f].long()
        rmask = torch.ones(1, 1, 33, dtype=torch.bool); rmask[0, 0, 32] = False
        m.prefill(row, rmask, torch.tensor([[S + f]]))
    print(f"tiny teacher-forced: max|dlogit|={max_diff:.4f} (oracle bf16-vs-fp32 gap {noise:.4f}); mismatches {mism}")
    assert max_diff <= 1.25 * noise
    for f, cb, margin in mism:
        _excuse(margin, noise, f"greedy index differs at frame {f} codebook {cb}", tie=2.0)


def test_tiny_batch_rows_independent(tiny):
    """B=3 identical prompts give 3 identical frames, equal to the B=1 result (batch slots
    share nothing)."""
    shape, w, m = tiny
    gold = torch.load(os.path.join(GOLD, "tiny_frames.pt"))
    tok, msk = gold["prompt_tokens"], gold["prompt_mask"]
    S = tok.shape[0]
    outs = []
    for B in (1, 3):
        m.reset_caches()
        m.prefill(tok.unsqueeze(0).repeat(B, 1, 1), msk.unsqueeze(0).repeat(B, 1, 1), torch.arange(S).unsqueeze(0).repeat(B, 1))
        o = [m.depth(B, 1.0, 1, commit=True).cpu()]
        for _ in range(3):
            m.step(B, 1.0, 1, use_graph=False)
            o.append(m.last_frame(B).cpu())
        outs.append(torch.stack(o))
    assert torch.equal(outs[1][:, 0], outs[1][:, 1]) and torch.equal(outs[1][:, 0], outs[1][:, 2])
    assert torch.equal(outs[0][:, 0], outs[1][:, 0])


def test_wide_batch_decode_matches_single_stream():
    """B = 16 identical prompts run the matrix-core (wide-M) decode path; every row must agree
    with the others bit-for-bit and with the B = 1 GEMV path / the golden logits within the
    rounding-noise floor (the two paths sum in different orders)."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from sesameai.models import Model, csm_tiny_args, synthetic_state_dict
    gold = torch.load(os.path.join(GOLD, "tiny_frames.pt"))
    tok, msk = gold["prompt_tokens"], gold["prompt_mask"]
    S = tok.shape[0]
    m = Model(csm_tiny_args(), synthetic_state_dict(csm_tiny_args(), seed=1234), max_frames=16, max_prefill_rows=16 * S)
    m.setup_caches(16)
    res = {}
    for B in (1, 16):
        m.reset_caches()
        m.prefill(tok.unsqueeze(0).repeat(B, 1, 1), msk.unsqueeze(0).repeat(B, 1, 1), torch.arange(S).unsqueeze(0).repeat(B, 1))
        forced = gold["codes"][0].unsqueeze(0).repeat(B, 1)
        out, logits = m.depth(B, 1.0, 1, forced=forced, want_logits=True, commit=False)
        res[B] = (out.cpu(), logits.float().cpu())
    o16, l16 = res[16]
    assert all(torch.equal(o16[0], o16[b]) for b in range(16)), "batch rows differ from each other"
    assert (l16[:, 0] - l16[:, 7]).abs().max() == 0
    d = (l16[:, 0] - res[1][1][:, 0]).abs().max().item()
    noise = float(gold["bf16_vs_fp32_gap"].max())
    print(f"wide (B=16) vs narrow (B=1) logits: max|d|={d:.4f} (noise floor {noise:.4f})")
    assert d <= noise
    d = (l16[:, 0] - gold["logits"][0].float()).abs().max().item()
    assert d <= 1.25 * noise
    for cb in (o16[0] != gold["codes"][0]).nonzero().flatten().tolist():
        assert float(gold["margin"][0, cb]) <= 2 * noise


def test_tiny_graph_replay_equals_eager_and_oracle_free_run(tiny):
    """The hipGraph-captured frame step is bit-identical to eager launches, the history /
    EOS bookkeeping matches, and the greedy free-running trace equals the oracle's while no
    near-tie has been hit."""
    from oracle import csm_ref as C
    from sesameai.generator import Generator
    shape, w, m = tiny
    gold = torch.load(os.path.join(GOLD, "tiny_frames.pt"))
    gen = Generator.__new__(Generator)
    gen._model, gen.device, gen._eos_poll, gen._audio_tokenizer, gen._text_tokenizer = m, m.device, 4, None, None
    traces = []
    for use_graph in (False, True):
        m.reset_caches()
        S = gold["prompt_tokens"].shape[0]
        m.prefill(gold["prompt_tokens"].unsqueeze(0), gold["prompt_mask"].unsqueeze(0), torch.arange(S).unsqueeze(0))
        m.depth(1, 1.0, 1, commit=True)
        for _ in range(9):
            m.step(1, 1.0, 1, use_graph=use_graph)
        fr, eos = m.read_frames(1)
        assert fr.shape == (10, 1, 32) and int(eos[0]) == -1
        traces.append(fr[:, 0])
    assert torch.equal(traces[0], traces[1]), "graph replay differs from eager launches"
    frames = gen.generate_codes(gold["prompt_tokens"], gold["prompt_mask"], 10, 1.0, 1)
    assert torch.equal(frames[:, 0], traces[0])
    # The free-running trace must equal the LIVE oracle's (this host's CPU kernels; a golden trajectory is host-dependent
    # at near-ties) up to, not including, the first frame in which the oracle's own top-1/top-2 margin drops under the
    # rounding-noise floor (2 x its bf16-vs-fp32 gap) -- before that frame nothing is free.
    om = C.OracleModel(shape, w); om.setup_caches(1)
    noise = float(gold["bf16_vs_fp32_gap"].max())
    cur_t, cur_m = gold["prompt_tokens"].unsqueeze(0), gold["prompt_mask"].unsqueeze(0)
    pos = torch.arange(cur_t.shape[1]).unsqueeze(0)
    ref, first_tie = [], None
    for f in range(10):
        tr = C.FrameTrace()
        sframe = om.generate_frame(cur_t, cur_m, pos, 1.0, 1, greedy=True, trace=tr)
        top2 = torch.topk(torch.stack(tr.logits, 0)[:, 0].float(), 2, dim=-1)[0]
        if first_tie is None and bool(((top2[:, 0] - top2[:, 1]) <= 2 * noise).any()):
            first_tie = f
        ref.append(sframe[0])
        cur_t = torch.cat([sframe.long(), torch.zeros(1, 1).long()], dim=1).unsqueeze(1)
        cur_m = torch.cat([torch.ones_like(sframe).bool(), torch.zeros(1, 1).bool()], dim=1).unsqueeze(1)
        pos = pos[:, -1:] + 1
    ref = torch.stack(ref)
    first_tie = 10 if first_tie is None else first_tie
    same = (ref == traces[0]).all(dim=1)
    n_same = int(same.float().cumprod(0).sum())
    print(f"free-running greedy: first {n_same}/10 frames identical to the oracle; the oracle's first near-tie is in frame {first_tie}")
    assert n_same >= first_tie, (n_same, first_tie)
    # a frame that differs must part at a codebook where the oracle's margin is inside the noise floor
    if n_same < 10:
        f = n_same
        om2 = C.OracleModel(shape, w); om2.setup_caches(1)
        cur_t, cur_m = gold["prompt_tokens"].unsqueeze(0), gold["prompt_mask"].unsqueeze(0)
        pos = torch.arange(cur_t.shape[1]).unsqueeze(0)
        for g in range(f + 1):
            tr = C.FrameTrace()
            sframe = om2.generate_frame(cur_t, cur_m, pos, 1.0, 1, greedy=True, trace=tr)
            cur_t = torch.cat([sframe.long(), torch.zeros(1, 1).long()], dim=1).unsqueeze(1)
            cur_m = torch.cat([torch.ones_like(sframe).bool(), torch.zeros(1, 1).bool()], dim=1).unsqueeze(1)
            pos = pos[:, -1:] + 1
        top2 = torch.topk(torch.stack(tr.logits, 0)[:, 0].float(), 2, dim=-1)[0]
        _same_until_a_near_tie(traces[0][f], ref[f], top2[:, 0] - top2[:, 1], noise, f"free run, frame {f}", tie=2.0)


def test_frame_graphs_are_kept_per_batch_and_sampling_parameters(tiny):
    """csm_frame_step keeps up to 4 captured frame steps, keyed on (B, top-k, temperature), least recently used replaced first (VERDICT r5
    missing #7: until round 5 ONE graph, so a service alternating the reference's 0.7/30, 0.8/40, 0.9/50 -- tts_service.py:175,266 --
    re-captured 40-151 nodes per switch).  A sequence of steps that alternates four keys captures four times, then never again; a
    fifth key evicts the least recently used one; and the frames are bit-identical to the same sequence launched eagerly."""
    from sesameai.models import Model, csm_tiny_args
    shape, w, _ = tiny
    gold = torch.load(os.path.join(GOLD, "tiny_frames.pt"))
    from sesameai.models import synthetic_state_dict
    m = Model(csm_tiny_args(), synthetic_state_dict(csm_tiny_args(), seed=1234), max_frames=64, max_prefill_rows=256)
    m.setup_caches(4)
    tok, msk = gold["prompt_tokens"], gold["prompt_mask"]
    S = tok.shape[0]
    keys = [(4, 0.7, 30), (4, 0.9, 50), (1, 0.7, 30), (4, 0.8, 40)]
    plan = keys * 3 + [(2, 0.7, 30)] + keys[1:] + [keys[0]]
    runs = []
    for use_graph in (True, False):
        m.reset_caches(); m.seed(99)
        m.prefill(tok.unsqueeze(0).repeat(4, 1, 1), msk.unsqueeze(0).repeat(4, 1, 1), torch.arange(S).unsqueeze(0).repeat(4, 1))
        m.depth(4, 0.7, 30, commit=True)
        c0 = m.graph_captures()
        seen = []
        for (B, T, k) in plan:
            m.step(B, T, k, use_graph=use_graph)
            seen.append(m.graph_captures() - c0)
        fr, _ = m.read_frames(4)
        runs.append((fr, seen))
    (fg, seen_g), (fe, seen_e) = runs
    assert torch.equal(fg, fe), "replayed graphs and eager launches of the same step sequence differ"
    assert seen_e == [0] * len(plan), "eager steps must not capture"
    assert seen_g[:4] == [1, 2, 3, 4] and seen_g[4:12] == [4] * 8, f"re-captured on a revisited key: {seen_g}"
    # the fifth key replaced the least recently used entry, keys[0]; keys[1:] still replay; keys[0] comes back with one more capture
    assert seen_g[12] == 5 and seen_g[13:16] == [5, 5, 5] and seen_g[16] == 6, seen_g
    assert "frame_graphs=LRU of 4" in m.describe()


def test_randomised_batch_length_and_prefill_form_vs_live_oracle(tiny):
    """tools/soak_parity.py's randomised cases inside the suite, at a fixed seed: 12 random (batch, prompt length,
    prompt-mode / plain prefill) combinations -- GEMV rows, 32 x 32 matrix-core tiles, the several-tiles-per-wave prompt kernels, flash
    and per-row attention -- each followed by two teacher-forced frames, FULL logits [32][B][V] against the LIVE oracle.  Bound: the tool's,
    2 x the oracle's bf16-vs-fp32 gap on the tiny shapes (0.018: less than one bf16 ulp of a logit >= 2, and these are maxima over
    65,632 x B logits per frame, not over the top-8 of a row; measured 0.0234 = 1.29 x = three half-ulps, profiles/r05/soak_parity.txt and r06)."""
    import random
    from oracle import csm_ref as C
    from sesameai.models import Model, csm_tiny_args, synthetic_state_dict
    shape, w, _ = tiny
    gold = torch.load(os.path.join(GOLD, "tiny_frames.pt"))
    noise = float(gold["bf16_vs_fp32_gap"].max())
    m = Model(csm_tiny_args(), synthetic_state_dict(csm_tiny_args(), seed=1234), max_frames=16, max_prefill_rows=1400)
    m.setup_caches(8)
    m.prefix_reuse = False
    rng = random.Random(7)
    worst, cases = 0.0, []
    for case in range(12):
        B = rng.choice([1, 1, 2, 3, 4, 7, 8])
        S = rng.choice([1, 2, 3, 5, 17, 31, 32, 33, 64, 65, 100, 127, 129, 160, 170])
        prompt = rng.random() < 0.5
        g = torch.Generator().manual_seed(1000 + case)
        nt = min(S, rng.randint(0, 6))
        tok = torch.zeros(B, S, 33, dtype=torch.long); msk = torch.zeros(B, S, 33, dtype=torch.bool)
        tok[:, :nt, 32] = torch.randint(0, shape.text_vocab_size, (B, nt), generator=g); msk[:, :nt, 32] = True
        tok[:, nt:, :32] = torch.randint(0, 2048, (B, S - nt, 32), generator=g); msk[:, nt:, :32] = True
        pos = torch.arange(S).unsqueeze(0).repeat(B, 1)
        m.reset_caches()
        if prompt:
            m.prefill_prompt(tok, msk)
        else:
            m.prefill(tok, msk, pos)
        om = C.OracleModel(shape, w); om.setup_caches(B)
        cur_t, cur_m, cur_p = tok, msk, pos
        for f in range(2):
            tr = C.FrameTrace()
            ref = om.generate_frame(cur_t, cur_m, cur_p, 1.0, 1, greedy=True, trace=tr)
            want = torch.stack(tr.logits, 0).float()                              # [32][B][V]
            out, logits = m.depth(B, 1.0, 1, forced=ref, want_logits=True, commit=False)
            d = (logits.float().cpu() - want).abs().max().item()
            worst = max(worst, d)
            assert d <= 2.0 * noise, f"case {case} B={B} S={S} prompt={prompt} frame {f}: max|dlogit| {d:.4f} > 2 x {noise:.4f}"
            cur_t = torch.cat([ref.long(), torch.zeros(B, 1).long()], dim=1).unsqueeze(1)
            cur_m = torch.cat([torch.ones_like(ref).bool(), torch.zeros(B, 1).bool()], dim=1).unsqueeze(1)
            cur_p = cur_p[:, -1:] + 1
            m.prefill(cur_t, cur_m, cur_p)
        cases.append((B, S, int(prompt)))
    print(f"\n[soak] 12 randomised (B, S, prompt-mode) cases {cases}: worst max|dlogit| {worst:.4f} = {worst / noise:.2f} x gap")


def test_generate_frame_surface_matches_reference_loop(tiny):
    """Driving Model.generate_frame exactly like the reference loop does
    (sesameai/generator.py:283-294 / tts_service.py:224-241) equals the fused on-device loop."""
    shape, w, m = tiny
    gold = torch.load(os.path.join(GOLD, "tiny_frames.pt"))
    tok, msk = gold["prompt_tokens"].cuda(), gold["prompt_mask"].cuda()
    m.reset_caches()
    curr_tokens, curr_mask = tok.unsqueeze(0), msk.unsqueeze(0)
    curr_pos = torch.arange(0, tok.size(0)).unsqueeze(0).long().cuda()
    samples = []
    for _ in range(5):
        sample = m.generate_frame(curr_tokens, curr_mask, curr_pos, 1.0, 1)
        assert sample.shape == (1, 32) and sample.dtype == torch.int32
        samples.append(sample)
        curr_tokens = torch.cat([sample, torch.zeros(1, 1).long().cuda()], dim=1).unsqueeze(1)
        curr_mask = torch.cat([torch.ones_like(sample).bool(), torch.zeros(1, 1).bool().cuda()], dim=1).unsqueeze(1)
        curr_pos = curr_pos[:, -1:] + 1
    got = torch.cat(samples).cpu()
    m.reset_caches()
    m.prefill(tok.unsqueeze(0), msk.unsqueeze(0), torch.arange(tok.size(0)).unsqueeze(0))
    m.depth(1, 1.0, 1, commit=True)
    for _ in range(4):
        m.step(1, 1.0, 1)
    fr, _ = m.read_frames(1)
    assert torch.equal(got, fr[:, 0])


def test_generate_frame_one_call_entry_equals_the_three_call_path_for_every_input_form(tiny):
    """csm_generate_frame_s1 (include/csm_hip.h): the reference's own tensors -- int64 tokens / positions, bool mask, on the GPU --
    are read by the staging kernel as they are.  Same frames as (a) csm_set_step_inputs + csm_frame_step + csm_copy_frame with
    converted int32 / uint8 inputs and (b) generate_frame fed host tensors of other dtypes (the binding converts), at B = 1 and 3."""
    import ctypes as C
    from sesameai import _abi
    shape, w, m = tiny
    for B in (1, 3):
        prs = [_tiny_prompt(10, 300 + b) for b in range(B)]
        tok, msk = torch.stack([p[0] for p in prs]).cuda(), torch.stack([p[1] for p in prs]).cuda()
        S = tok.shape[1]

        def run(form):
            m.reset_caches()
            f = m.generate_frame(tok, msk, torch.arange(S).unsqueeze(0).repeat(B, 1).cuda(), 1.0, 1)
            out = [f.cpu()]
            pos = torch.full((B, 1), S, dtype=torch.long)
            for _ in range(4):
                t = torch.cat([f.long(), torch.zeros(B, 1, dtype=torch.long, device=f.device)], dim=1).unsqueeze(1)
                k = torch.cat([torch.ones_like(f).bool(), torch.zeros(B, 1, dtype=torch.bool, device=f.device)], dim=1).unsqueeze(1)
                if form == "reference":                                     # int64 / bool / int64 on the device: no conversion
                    f = m.generate_frame(t, k, pos.cuda(), 1.0, 1)
                elif form == "host":                                        # int32 / uint8 host tensors: the binding converts
                    f = m.generate_frame(t.cpu().int(), k.cpu().to(torch.uint8), pos.int(), 1.0, 1)
                else:                                                       # the three-call path of rounds 1-3
                    ti, ki, pi = t.int().contiguous(), k.to(torch.uint8).contiguous(), pos.int().cuda().contiguous()
                    _abi.check(_abi.lib.csm_set_step_inputs(m._h, ti.data_ptr(), ki.data_ptr(), pi.data_ptr(), B, torch.cuda.current_stream().cuda_stream), m._h)
                    m.step(B, 1.0, 1)
                    f = m.last_frame(B)
                assert f.shape == (B, 32) and f.dtype == torch.int32 and f.is_cuda
                out.append(f.cpu()); pos = pos + 1
            return torch.stack(out)

        ref, host, three = run("reference"), run("host"), run("three")
        assert torch.equal(ref, three) and torch.equal(ref, host), f"B = {B}"
        fr, _ = m.read_frames(B)
        assert torch.equal(fr, three), "history"
    # a position outside [0, max_seq) that only exists on the device is reported at the next read_frames, as in the three-call path
    m.reset_caches()
    f = m.generate_frame(tok[:1], msk[:1], torch.arange(S).unsqueeze(0).cuda(), 1.0, 1)
    t = torch.cat([f.long(), torch.zeros(1, 1, dtype=torch.long, device=f.device)], dim=1).unsqueeze(1)
    k = torch.cat([torch.ones_like(f).bool(), torch.zeros(1, 1, dtype=torch.bool, device=f.device)], dim=1).unsqueeze(1)
    m.generate_frame(t, k, torch.tensor([[256]]).cuda(), 1.0, 1)
    with pytest.raises(RuntimeError, match="CSM_E_TOO_LONG"):
        m.read_frames(1)
    with pytest.raises(ValueError, match="input_pos outside"):
        m.generate_frame(t, k, torch.tensor([[256]]), 1.0, 1)               # host positions are checked before anything is launched
    m.reset_caches()


def test_frame_history_is_a_ring_and_overwritten_frames_are_refused():
    """the history was linear and a long continuous run ended in CSM_E_TOO_LONG.  With max_frames = 8 a run of 29 frames
    read in blocks of 4 returns exactly the frames of a run with a large history; a range that has been overwritten is refused."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from sesameai.models import Model, csm_tiny_args, synthetic_state_dict
    sd = synthetic_state_dict(csm_tiny_args(), seed=1234)
    tok, msk = _tiny_prompt(10, 77)
    runs = []
    for max_frames in (8, 64):
        m = Model(csm_tiny_args(), sd, max_frames=max_frames, max_prefill_rows=64)
        m.setup_caches(2)
        m.reset_caches()
        m.prefill(torch.stack([tok, tok]), torch.stack([msk, msk]), torch.arange(10).unsqueeze(0).repeat(2, 1))
        m.depth(2, 1.0, 1, commit=True)
        got, first = [m.read_frames(2, 0, 1)[0]], 1
        for _ in range(7):
            for _ in range(4):
                m.step(2, 1.0, 1)
            got.append(m.read_frames(2, first, 4)[0]); first += 4
        runs.append(torch.cat(got))
        if max_frames == 8:
            assert m.num_frames() == 29
            assert torch.equal(m.read_frames(2, 21, 8)[0], runs[0][21:29])          # the whole ring, across the wrap
            with pytest.raises(RuntimeError, match="overwritten"):
                m.read_frames(2, 20, 4)
        del m
    assert runs[0].shape == (29, 2, 32) and torch.equal(runs[0], runs[1])


def test_prefix_kv_reuse_is_bit_identical(tiny):
    """second sentence with the same voice-prompt context: only the rows after the common prefix
    are prefilled, and the generated frames equal those of a cold full prefill."""
    from sesameai.generator import Generator
    shape, w, m = tiny
    gen = Generator.__new__(Generator)
    gen._model, gen.device, gen._eos_poll, gen._audio_tokenizer, gen._text_tokenizer = m, m.device, 4, None, None
    g = torch.Generator().manual_seed(21)
    ctx_t = torch.zeros(40, 33, dtype=torch.long); ctx_m = torch.zeros(40, 33, dtype=torch.bool)
    ctx_t[:10, 32] = torch.randint(0, 1000, (10,), generator=g); ctx_m[:10, 32] = True
    ctx_t[10:, :32] = torch.randint(0, 2048, (30, 32), generator=g); ctx_m[10:, :32] = True

    def prompt(n_text, seed):
        t = torch.zeros(n_text, 33, dtype=torch.long); mk = torch.zeros(n_text, 33, dtype=torch.bool)
        t[:, 32] = torch.randint(0, 1000, (n_text,), generator=torch.Generator().manual_seed(seed)); mk[:, 32] = True
        return torch.cat([ctx_t, t]), torch.cat([ctx_m, mk])

    p1, p2 = prompt(5, 1), prompt(7, 2)
    m.prefix_reuse = True
    m._kv_prompt = None
    gen.generate_codes(*p1, 6, 1.0, 1)
    assert m.last_prefill_rows == 45
    warm = gen.generate_codes(*p2, 6, 1.0, 1)
    assert m.last_prefill_rows == 7, "only the new text rows should have been prefilled"
    m.prefix_reuse = False
    cold = gen.generate_codes(*p2, 6, 1.0, 1)
    assert m.last_prefill_rows == 47
    m.prefix_reuse = True
    assert torch.equal(warm, cold)
    # identical prompt again: one row (the last) still runs to produce last_h
    again = gen.generate_codes(*p2, 6, 1.0, 1)
    assert m.last_prefill_rows == 1 and torch.equal(again, cold)


def test_prompt_inputs_from_the_host_equal_device_inputs(tiny):
    """Model._to_dev: host prompt tensors are cast by one numpy pass into the model's pinned staging buffer and copied asynchronously
    (no torch CPU kernel, no pageable copy).  Whatever the caller hands over -- int64 / int32, bool / uint8, contiguous or a strided
    view, on the host or on the device -- the frame is the same; many prompts in a row wrap the staging buffer."""
    shape, w, m = tiny
    B, S = 2, 14
    pr = [_tiny_prompt(S, 70 + b) for b in range(B)]
    tok, msk = torch.stack([p[0] for p in pr]), torch.stack([p[1] for p in pr])
    pos = torch.arange(S).unsqueeze(0).repeat(B, 1)

    def frame(t, k, p):
        m.reset_caches(); m.seed(3)
        m.prefill(t, k, p)
        return m.depth(B, 1.0, 1, commit=True).clone()

    want = frame(tok.cuda(), msk.cuda(), pos.cuda())
    wide_t = torch.zeros(B, S, 66, dtype=torch.long); wide_t[:, :, ::2] = tok          # a strided view of a wider host tensor
    forms = [(tok, msk, pos), (tok.int(), msk.to(torch.uint8), pos.int()), (wide_t[:, :, ::2], msk, pos),
             (tok, msk.cuda(), pos), (tok.cuda().int(), msk, pos.cuda())]
    for t, k, p in forms:
        assert torch.equal(frame(t, k, p), want)
    for i in range(260):                                      # ~5 KB staged per prompt: more than once around the 1 MiB ring
        m.reset_caches(); m.prefill(tok, msk, pos)
    assert torch.equal(frame(tok, msk, pos), want)
    big = torch.zeros(1, 200, 33, dtype=torch.long); big[0, :, 32] = 5
    bm = torch.zeros(1, 200, 33, dtype=torch.bool); bm[0, :, 32] = True
    m.reset_caches(); m.prefill(big, bm, torch.arange(200).unsqueeze(0))               # a larger prompt than anything staged so far
    assert torch.equal(frame(tok, msk, pos), want)


def test_prompt_too_long_raises(tiny):
    from sesameai.generator import Generator
    shape, w, m = tiny
    gen = Generator.__new__(Generator)
    gen._model, gen.device, gen._eos_poll = m, m.device, 4
    tok = torch.zeros(1700, 33, dtype=torch.long); msk = torch.zeros(1700, 33, dtype=torch.bool); msk[:, 32] = True
    with pytest.raises(ValueError, match="Inputs too long"):
        gen.generate_codes(tok, msk, int(30_000 / 80), 0.9, 50)      # 1700 >= 2048 - 375


def test_fp8_weight_stream_matches_oracle_on_dequantised_weights():
    """BASELINE config 5: the decode step streams OCP-e4m3 weights with power-of-two row scales.
    byte*scale is exactly the bf16 value the oracle holds, so the fp8 path must agree with the
    oracle on those dequantised weights to the same tolerance as the bf16 path does."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from oracle import csm_ref as C
    from sesameai.models import Model, csm_tiny_args, fp8_weight_set, synthetic_state_dict
    shape = C.csm_tiny()
    w = C.fp8_dequantized(C.make_weights(shape, seed=1234))
    sd = synthetic_state_dict(csm_tiny_args(), seed=1234)
    deq, _ = fp8_weight_set(csm_tiny_args(), sd)
    assert all(torch.equal(w[k], deq[k]) for k in w), "product and oracle fp8 dequantisation differ"
    gold = torch.load(os.path.join(GOLD, "tiny_frames.pt"))
    tok, msk = gold["prompt_tokens"], gold["prompt_mask"]
    S = tok.shape[0]
    m = Model(csm_tiny_args(), sd, max_frames=16, max_prefill_rows=64, weights_dtype="fp8")
    m.setup_caches(1)
    om = C.OracleModel(shape, w); om.setup_caches(1)
    m.prefill(tok.unsqueeze(0), msk.unsqueeze(0), torch.arange(S).unsqueeze(0))
    cur_t, cur_m, pos = tok.unsqueeze(0), msk.unsqueeze(0), torch.arange(S).unsqueeze(0)
    noise = float(gold["bf16_vs_fp32_gap"].max())
    worst = 0.0
    for f in range(4):
        tr = C.FrameTrace()
        ref = om.generate_frame(cur_t, cur_m, pos, 1.0, 1, greedy=True, trace=tr)
        want = torch.stack(tr.logits, 0)[:, 0].float()
        out, logits = m.depth(1, 1.0, 1, forced=ref, want_logits=True, commit=False)
        worst = max(worst, (logits[:, 0].float().cpu() - want).abs().max().item())
        margin = torch.topk(want, 2, dim=-1)[0]
        for cb in (out[0].cpu() != ref[0]).nonzero().flatten().tolist():
            _excuse(float(margin[cb, 0] - margin[cb, 1]), noise, f"CSM-1B config-1 frame {f} codebook {cb}")
        cur_t = torch.cat([ref.long(), torch.zeros(1, 1).long()], dim=1).unsqueeze(1)
        cur_m = torch.cat([torch.ones_like(ref).bool(), torch.zeros(1, 1).bool()], dim=1).unsqueeze(1)
        pos = pos[:, -1:] + 1
        m.prefill(cur_t, cur_m, pos)                                 # S == 1: the narrow fp8 GEMV path
    print(f"fp8 weight stream vs oracle(dequantised): max|dlogit|={worst:.4f} (noise floor {noise:.4f})")
    assert worst <= 1.25 * noise


def test_long_context_streaming_config5_shape():
    """BASELINE config 5 shape at CSM-1B size (bf16 here): 10 prompt segments -> S = 1334 rows,
    375 frames (30 s), Mimi decoded statefully every 10 frames.  Checks the position guard
    (1334 + 375 <= 2048), that the run completes without EOS on random weights, and that the
    streamed audio equals the whole-utterance decode of the same codes."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from sesameai.generator import Generator
    from sesameai.mimi import MimiArgs, MimiCodec
    from sesameai.models import Model, csm_1b_args
    g = torch.Generator().manual_seed(5)
    rows_t, rows_m = [], []
    for seg in range(10):
        t = torch.zeros(131, 33, dtype=torch.long); mk = torch.zeros(131, 33, dtype=torch.bool)
        t[:30, 32] = torch.randint(0, 128256, (30,), generator=g); mk[:30, 32] = True
        t[30:130, :32] = torch.randint(0, 2048, (100, 32), generator=g); mk[30:, :32] = True      # + EOS row
        rows_t.append(t); rows_m.append(mk)
    t = torch.zeros(24, 33, dtype=torch.long); mk = torch.zeros(24, 33, dtype=torch.bool)
    t[:, 32] = torch.randint(0, 128256, (24,), generator=g); mk[:, 32] = True
    tok, msk = torch.cat(rows_t + [t]), torch.cat(rows_m + [mk])
    assert tok.shape[0] == 1334
    model = Model(csm_1b_args(), None, max_frames=400, max_prefill_rows=1400)
    codec = MimiCodec(MimiArgs(), None, max_frames=400)
    gen = Generator(model, audio_tokenizer=codec)
    model.seed(11)
    chunks = []
    codec.reset_stream()

    def on_frames(fr):                                            # fr: [n][1][32] -> stateful Mimi stream
        chunks.append(codec.decode_stream(fr.permute(1, 2, 0).contiguous()))

    frames = gen.generate_codes(tok, msk, 375, 0.9, 50, on_frames=on_frames, poll=10)
    assert frames.shape == (375, 1, 32) and int(gen.last_eos_at[0]) == -1
    streamed = torch.cat(chunks, dim=-1)
    whole = codec.decode(frames.permute(1, 2, 0).contiguous())
    assert streamed.shape == whole.shape == (1, 1, 375 * 1920)
    assert (streamed - whole).abs().max().item() <= 1e-5 * whole.abs().max().item()
    with pytest.raises(ValueError, match="Inputs too long"):
        gen.generate_codes(tok, msk, 2048 - 1334, 0.9, 50)         # S >= 2048 - max_generation_len


@pytest.fixture(scope="module")
def csm1b():
    """(golden, seeded CSM-1B state dict on the host) shared by the full-size tests."""
    path = os.path.join(GOLD, "csm1b_frames.pt")
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    if not os.path.exists(path):
        pytest.skip("csm1b golden not generated")
    from sesameai.models import csm_1b_args, synthetic_state_dict
    gold = torch.load(path)
    return gold, synthetic_state_dict(csm_1b_args(), seed=int(gold["weight_seed"]))


def test_csm1b_teacher_forced_vs_golden(csm1b):
    """Full CSM-1B shapes, seeded weights: logits (top-8 per row) and greedy indices for every
    codebook of every golden frame, teacher-forced on the oracle's trajectory."""
    from sesameai.models import Model, csm_1b_args
    gold, sd = csm1b
    m = Model(csm_1b_args(), sd, max_frames=64, max_prefill_rows=256)
    m.setup_caches(1)
    tok, msk = gold["prompt_tokens"], gold["prompt_mask"]
    S = tok.shape[0]
    noise = float(gold["bf16_vs_fp32_gap"].max())
    m.prefill(tok.unsqueeze(0), msk.unsqueeze(0), torch.arange(S).unsqueeze(0))
    max_diff, mism = 0.0, []
    for f in range(gold["codes"].shape[0]):
        forced = gold["codes"][f].unsqueeze(0)
        out, logits = m.depth(1, 1.0, 1, forced=forced, want_logits=True, commit=False)
        lg = logits[:, 0].float().cpu()
        d = (torch.gather(lg, 1, gold["top_i"][f].long()) - gold["top_v"][f].float()).abs().max().item()
        max_diff = max(max_diff, d)
        for cb in (out[0].cpu() != gold["codes"][f]).nonzero().flatten().tolist():
            mism.append((f, cb, float(gold["margin"][f, cb])))
        row = torch.zeros(1, 1, 33, dtype=torch.long); row[0, 0, :32] = gold["codes"][f].long()
        rmask = torch.ones(1, 1, 33, dtype=torch.bool); rmask[0, 0, 32] = False
        m.prefill(row, rmask, torch.tensor([[S + f]]))
    n_rows = 32 * gold["codes"].shape[0]
    print(f"csm-1b teacher-forced: max|dlogit|={max_diff:.4f} (oracle bf16-vs-fp32 gap {noise:.4f}); {len(mism)} of {n_rows} greedy rows excused as near-ties "
          f"({100.0 * len(mism) / n_rows:.1f} %): {mism}")
    assert max_diff <= noise
    assert len(mism) <= 0.08 * n_rows, "too many greedy rows differ from the oracle, near-ties or not" 
    for f, cb, margin in mism:
        _excuse(margin, noise, f"greedy index differs at frame {f} codebook {cb}")


def test_csm1b_batched_wide_path_vs_golden(csm1b):
    """Full size, B = 4 identical utterances: every row takes the matrix-core (wide) path in BOTH stacks; rows must be
    bit-identical to each other (no cross-row coupling) and match the oracle's golden logits like the B = 1 path."""
    from sesameai.models import Model, csm_1b_args
    gold, sd = csm1b
    B = 4
    m = Model(csm_1b_args(), sd, max_frames=16, max_prefill_rows=B * 256)
    m.setup_caches(B)
    tok, msk = gold["prompt_tokens"], gold["prompt_mask"]
    S = tok.shape[0]
    noise = float(gold["bf16_vs_fp32_gap"].max())
    m.prefill(tok.unsqueeze(0).repeat(B, 1, 1), msk.unsqueeze(0).repeat(B, 1, 1), torch.arange(S).unsqueeze(0).repeat(B, 1))
    max_diff = 0.0
    for f in range(3):
        forced = gold["codes"][f].unsqueeze(0).repeat(B, 1)
        out, logits = m.depth(B, 1.0, 1, forced=forced, want_logits=True, commit=False)      # logits [32][B][V]
        for b in range(1, B):
            assert torch.equal(logits[:, b], logits[:, 0]) and torch.equal(out[b], out[0])
        lg = logits[:, 0].float().cpu()
        max_diff = max(max_diff, (torch.gather(lg, 1, gold["top_i"][f].long()) - gold["top_v"][f].float()).abs().max().item())
        for cb in (out[0].cpu() != gold["codes"][f]).nonzero().flatten().tolist():
            _excuse(float(gold["margin"][f, cb]), noise, f"greedy index differs at frame {f} codebook {cb}")
        row = torch.zeros(B, 1, 33, dtype=torch.long); row[:, 0, :32] = gold["codes"][f].long()
        rmask = torch.ones(B, 1, 33, dtype=torch.bool); rmask[:, 0, 32] = False
        m.prefill(row, rmask, torch.full((B, 1), S + f))
    print(f"csm-1b B=4 wide path: max|dlogit|={max_diff:.4f} (gap {noise:.4f})")
    assert max_diff <= noise


def test_csm1b_prefix_reuse_bit_identical(csm1b):
    """Full size: a follow-up sentence prefills only its new rows and generates exactly the frames of a cold prefill
    (the split-K grouping of prompt rows is a function of K alone, never of the row count)."""
    from sesameai.generator import Generator
    from sesameai.models import Model, csm_1b_args
    gold, sd = csm1b
    m = Model(csm_1b_args(), sd, max_frames=16, max_prefill_rows=256)
    m.setup_caches(1)
    gen = Generator.__new__(Generator)
    gen._model, gen.device, gen._eos_poll, gen._audio_tokenizer, gen._text_tokenizer = m, m.device, 4, None, None
    g = torch.Generator().manual_seed(5)
    ctx_t = torch.zeros(150, 33, dtype=torch.long); ctx_m = torch.zeros(150, 33, dtype=torch.bool)
    ctx_t[:30, 32] = torch.randint(0, 128256, (30,), generator=g); ctx_m[:30, 32] = True
    ctx_t[30:, :32] = torch.randint(0, 2048, (120, 32), generator=g); ctx_m[30:, :32] = True

    def prompt(n_text, seed):
        t = torch.zeros(n_text, 33, dtype=torch.long); mk = torch.zeros(n_text, 33, dtype=torch.bool)
        t[:, 32] = torch.randint(0, 128256, (n_text,), generator=torch.Generator().manual_seed(seed)); mk[:, 32] = True
        return torch.cat([ctx_t, t]), torch.cat([ctx_m, mk])

    p1, p2 = prompt(20, 1), prompt(24, 2)
    m.prefix_reuse = True
    m._kv_prompt = None
    gen.generate_codes(*p1, 3, 1.0, 1)
    warm = gen.generate_codes(*p2, 3, 1.0, 1)
    assert m.last_prefill_rows == 24
    m.prefix_reuse = False
    cold = gen.generate_codes(*p2, 3, 1.0, 1)
    assert m.last_prefill_rows == 174
    assert torch.equal(warm, cold)


def test_long_prompt_kernel_keeps_rows_independent_of_row_count():
    """Tiny shapes: 5 x 80 = 400 prompt rows take the 128 x 128 LDS-tiled kernels (M >= 256), 3 x 80 = 240 rows the
    32 x 32 ones; the logits and frames of the shared utterances must be bit-identical (the guarantee behind
    prefix-KV reuse for prompts of any length)."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from sesameai.models import Model, csm_tiny_args, synthetic_state_dict
    m = Model(csm_tiny_args(), synthetic_state_dict(csm_tiny_args(), seed=1234), max_frames=16, max_prefill_rows=640)
    m.setup_caches(5)
    g = torch.Generator().manual_seed(77)
    S = 80
    tok = torch.zeros(5, S, 33, dtype=torch.long); msk = torch.zeros(5, S, 33, dtype=torch.bool)
    tok[:, :20, 32] = torch.randint(0, 1000, (5, 20), generator=g); msk[:, :20, 32] = True
    tok[:, 20:, :32] = torch.randint(0, 2048, (5, S - 20, 32), generator=g); msk[:, 20:, :32] = True
    res = []
    for B in (5, 3):
        m.reset_caches()
        m.prefix_reuse = False
        assert m.prefill_prompt(tok[:B], msk[:B]) == S
        out, logits = m.depth(B, 1.0, 1, want_logits=True, commit=True)
        for _ in range(3):
            m.step(B, 1.0, 1)
        frames, _ = m.read_frames(B)
        res.append((logits.cpu(), frames))
    assert torch.equal(res[0][0][:, :3], res[1][0]), "logits differ between the 400-row and the 240-row prefill"
    assert torch.equal(res[0][1][:, :3], res[1][1])


@pytest.mark.parametrize("checkpoint", ["bench", "jitter"])
def test_layer0_qkv_table_gives_the_same_bits_as_computing_it(monkeypatch, checkpoint):
    """The depth decoder's layer-0 q/k/v of steps >= 2 come from a table precomputed with the production kernel
    (csm_engine.hip build_qkv0_table); CSM_QKV0_TABLE=0 computes them per step.  Same logits, same frames, bit for bit,
    for B = 1 and B = 2 (the GEMV path).  The table is the one place decoder layer 0's sa_norm is applied at load time: the
    `jitter` checkpoint (oracle.csm_ref.norm_test_weights) has scales != 1, so a table built without them, or with another
    layer's, differs."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from oracle import csm_ref as C
    from sesameai.models import Model, csm_tiny_args, synthetic_state_dict
    sd = synthetic_state_dict(csm_tiny_args(), seed=1234) if checkpoint == "bench" else C.norm_test_weights(C.csm_tiny(), seed=1234)
    g = torch.Generator().manual_seed(3)
    S = 12
    tok = torch.zeros(2, S, 33, dtype=torch.long); msk = torch.zeros(2, S, 33, dtype=torch.bool)
    tok[:, :5, 32] = torch.randint(0, 1000, (2, 5), generator=g); msk[:, :5, 32] = True
    tok[:, 5:, :32] = torch.randint(0, 2048, (2, S - 5, 32), generator=g); msk[:, 5:, :32] = True
    res = {}
    for flag in ("1", "0"):
        monkeypatch.setenv("CSM_QKV0_TABLE", flag)
        m = Model(csm_tiny_args(), sd, max_frames=16, max_prefill_rows=64)
        m.setup_caches(2)
        out = []
        for B in (1, 2):
            m.reset_caches(); m.seed(11)
            m.prefill(tok[:B], msk[:B], torch.arange(S).unsqueeze(0).repeat(B, 1))
            _, logits = m.depth(B, 0.9, 50, want_logits=True, commit=True)
            for _ in range(3):
                m.step(B, 0.9, 50)
            out.append((logits.cpu(), m.read_frames(B)[0]))
        res[flag] = out
        del m
    for (l1, f1), (l0, f0) in zip(res["1"], res["0"]):
        assert torch.equal(l1, l0) and torch.equal(f1, f0)


def test_fp8_stream_on_the_batched_path_equals_its_bf16_dequantisation_bitwise(monkeypatch):
    """fp8 mode, B = 4 (matrix-core path): decode steps stream e4m3 bytes converted in registers, with the power-of-two
    row scale applied to the fp32 sum.  The bf16 weights of that mode ARE the dequantised bytes, so streaming either
    must give identical logits and frames (CSM_FP8_WIDE=0 keeps the bf16 stream)."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from sesameai.models import Model, csm_tiny_args, synthetic_state_dict
    sd = synthetic_state_dict(csm_tiny_args(), seed=1234)
    g = torch.Generator().manual_seed(8)
    B, S = 26, 12                                  # 26 rows per decode step: operand-order activations are on as well
    tok = torch.zeros(B, S, 33, dtype=torch.long); msk = torch.zeros(B, S, 33, dtype=torch.bool)
    tok[:, :6, 32] = torch.randint(0, 1000, (B, 6), generator=g); msk[:, :6, 32] = True
    tok[:, 6:, :32] = torch.randint(0, 2048, (B, S - 6, 32), generator=g); msk[:, 6:, :32] = True
    res = {}
    for flag in ("1", "0"):
        monkeypatch.setenv("CSM_FP8_WIDE", flag)
        m = Model(csm_tiny_args(), sd, max_frames=16, max_prefill_rows=B * S, weights_dtype="fp8")
        m.setup_caches(B)
        m.seed(5)
        m.prefill(tok, msk, torch.arange(S).unsqueeze(0).repeat(B, 1))
        _, logits = m.depth(B, 0.9, 50, want_logits=True, commit=True)
        for _ in range(3):
            m.step(B, 0.9, 50)
        res[flag] = (logits.cpu(), m.read_frames(B)[0])
        del m
    assert torch.equal(res["1"][0], res["0"][0]) and torch.equal(res["1"][1], res["0"][1])
    assert res["1"][0].float().abs().max() > 0


@pytest.mark.parametrize("B", [13, 40])
def test_operand_order_activations_are_a_pure_layout_change(monkeypatch, B):
    """Batched decode steps keep xn / attention output / SiLU*up in matrix-core operand order between the kernels of a
    layer (CSM_XPACK=0: row-major).  Same values in a different place: logits and frames must be bit-identical, for
    one row tile (B = 13: 26 rows in decoder step 1, the only packed step there) and for two with a ragged tail (B = 40)."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from sesameai.models import Model, csm_tiny_args, synthetic_state_dict
    sd = synthetic_state_dict(csm_tiny_args(), seed=1234)
    g = torch.Generator().manual_seed(B)
    S = 9
    tok = torch.zeros(B, S, 33, dtype=torch.long); msk = torch.zeros(B, S, 33, dtype=torch.bool)
    tok[:, :4, 32] = torch.randint(0, 1000, (B, 4), generator=g); msk[:, :4, 32] = True
    tok[:, 4:, :32] = torch.randint(0, 2048, (B, S - 4, 32), generator=g); msk[:, 4:, :32] = True
    res = {}
    for flag in ("1", "0"):
        monkeypatch.setenv("CSM_XPACK", flag)
        m = Model(csm_tiny_args(), sd, max_frames=16, max_prefill_rows=B * S)
        m.setup_caches(B)
        m.seed(5)
        m.prefill(tok, msk, torch.arange(S).unsqueeze(0).repeat(B, 1))
        _, logits = m.depth(B, 0.9, 50, want_logits=True, commit=True)
        for _ in range(3):
            m.step(B, 0.9, 50)
        res[flag] = (logits.cpu(), m.read_frames(B)[0])
        del m
    assert torch.equal(res["1"][0], res["0"][0]) and torch.equal(res["1"][1], res["0"][1])


# ----------------------------------------------------------------------------------------
# the loop's stop rule ON THE DEVICE (reference: sesameai/generator.py:285, tts_service.py:228): k_advance raises
# eos_at[b] at the first all-zero frame; Generator trims at it.  Random weights never emit such a frame, so the
# tests make one: a frame whose Exp(1) race is rigged (q[0] tiny, q[v > 0] huge) samples code 0 in every codebook.
# ----------------------------------------------------------------------------------------
def _rigged_frame(model, B, S, frame_idx, zero_rows, T=1.0):
    """Frame `frame_idx` >= 1 by hand: one backbone row per sequence (the previous frame at position S + frame_idx - 1)
    through csm_prefill, then csm_depth with a noise tensor that makes sequences `zero_rows` sample all zeros."""
    V = model.config.audio_vocab_size
    dev = model.device
    prev = model.last_frame(B).long()
    tok = torch.zeros(B, 1, 33, dtype=torch.long, device=dev); tok[:, 0, :32] = prev
    msk = torch.zeros(B, 1, 33, dtype=torch.bool, device=dev); msk[:, 0, :32] = True
    pos = torch.full((B, 1), S + frame_idx - 1, dtype=torch.long)
    model.prefill(tok, msk, pos)
    g = torch.Generator().manual_seed(100 + frame_idx)
    noise = (0.05 + torch.rand(32, B, V, generator=g)).to(torch.bfloat16)
    for b in zero_rows:
        noise[:, b, :] = 1e30
        noise[:, b, 0] = 1e-30
    return model.depth(B, T, V, noise=noise, commit=True)


def _inject_eos(model, B, S, plan):
    """Replaces model.step so that frame k of sequence b is all-zero for every (k -> [b...]) of `plan`."""
    state = {"frame": 0}
    real_step, real_depth, real_reset = model.step, model.depth, model.reset_caches

    def reset():
        state["frame"] = 0
        real_reset()

    def depth(*a, **kw):
        out = real_depth(*a, **kw)
        if kw.get("commit", True) and not state.get("inside"):
            state["frame"] = 1                      # the prompt frame (index 0) exists now
        return out

    def step(batch, temperature, topk, use_graph=True):
        k = state["frame"]
        if k in plan:
            state["inside"] = True
            _rigged_frame(model, B, S, k, plan[k], T=1.0)
            state["inside"] = False
        else:
            real_step(batch, temperature, topk, use_graph)
        state["frame"] = k + 1

    model.step, model.depth, model.reset_caches = step, depth, reset
    return lambda: (setattr(model, "step", real_step), setattr(model, "depth", real_depth), setattr(model, "reset_caches", real_reset))


def test_device_side_eos_flag_and_trimming_b1(tiny):
    from sesameai.generator import Generator
    from oracle import csm_ref as C
    shape, w, m = tiny
    gen = Generator.__new__(Generator)
    gen._model, gen.device, gen._eos_poll, gen._stream_buffer_size, gen._mimi_stream = m, m.device, 4, 10, None
    g = torch.Generator().manual_seed(5)
    tok, msk = C.build_prompt([(torch.randint(0, shape.text_vocab_size, (9,), generator=g).tolist(), None)])
    S = tok.shape[0]
    for k in (1, 3, 4, 6, 11):                      # mid-block, last of a block, first of a block (poll = 4)
        undo = _inject_eos(m, 1, S, {k: [0]})
        try:
            m.seed(11)
            frames = gen.generate_codes(tok, msk, 20, 0.9, 50)
        finally:
            undo()
        allf, eos = m.read_frames(1)
        assert int(eos[0]) == k == int(gen.last_eos_at[0]), (k, eos)
        assert int(allf[k].abs().sum()) == 0 and int((allf[:k] != 0).any(dim=2).all()) == 1        # frame k is the all-zero one
        assert frames.shape == (k, 1, 32) and torch.equal(frames, allf[:k])                       # handed out: frames before it
        assert allf.shape[0] <= k + 1 + 2 * 4                                                     # and the loop stopped soon after


def test_device_side_eos_batch_of_three_different_stop_frames(tiny):
    from sesameai.generator import Generator
    from oracle import csm_ref as C
    shape, w, m = tiny
    gen = Generator.__new__(Generator)
    gen._model, gen.device, gen._eos_poll = m, m.device, 4
    g = torch.Generator().manual_seed(6)
    prompts = [C.build_prompt([(torch.randint(0, shape.text_vocab_size, (7,), generator=g).tolist(), None)]) for _ in range(3)]
    tok = torch.stack([p[0] for p in prompts]); msk = torch.stack([p[1] for p in prompts])
    S = tok.shape[1]
    undo = _inject_eos(m, 3, S, {2: [1], 5: [0], 9: [2]})
    try:
        m.seed(12)
        frames = gen.generate_codes(tok, msk, 30, 0.9, 50)
    finally:
        undo()
    assert gen.last_eos_at.tolist() == [5, 2, 9]
    assert 10 <= frames.shape[0] <= 10 + 2 * 4, frames.shape         # all three done at frame 9: stops within the enqueued blocks
    for b, k in enumerate([5, 2, 9]):
        assert int(frames[k, b].abs().sum()) == 0
        assert bool((frames[:k, b] != 0).any(dim=1).all())
    # a sequence that already stopped keeps its FIRST stop frame even if it emits zeros again
    undo = _inject_eos(m, 3, S, {2: [1], 4: [1, 0], 6: [2]})
    try:
        m.seed(13)
        gen.generate_codes(tok, msk, 30, 0.9, 50)
    finally:
        undo()
    assert gen.last_eos_at.tolist() == [4, 2, 6]


def test_zeroed_heads_stop_at_the_prompt_frame_and_generate_returns_empty_audio():
    """Advisor's case: head weights of zero -> every logit 0 -> greedy picks code 0 everywhere -> the very first frame is
    the EOS frame; Generator.generate returns torch.tensor([]) like the reference (generator.py:296-297)."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from sesameai.generator import Generator
    from sesameai.models import Model, csm_tiny_args, synthetic_state_dict
    sd = synthetic_state_dict(csm_tiny_args(), seed=1234)
    sd["codebook0_head.weight"] = torch.zeros_like(sd["codebook0_head.weight"])
    sd["audio_head"] = torch.zeros_like(sd["audio_head"])
    m = Model(csm_tiny_args(), sd, max_frames=32, max_prefill_rows=64)

    class Codec:
        sample_rate = 24_000
        def decode(self, codes): raise AssertionError("nothing to decode")

    gen = Generator(m, audio_tokenizer=Codec())
    audio = gen.generate([3, 4, 5, 6], 0, [], max_audio_length_ms=800, temperature=1.0, topk=1)
    assert audio.numel() == 0
    frames, eos = m.read_frames(1)
    assert int(eos[0]) == 0 and int(frames[0].abs().sum()) == 0
    assert list(gen.generate_stream([3, 4, 5, 6], 0, [], max_audio_length_ms=800, temperature=1.0, topk=1)) == []


def _tiny_prompt(rows, seed):
    g = torch.Generator().manual_seed(seed)
    t = torch.zeros(rows, 33, dtype=torch.long); m = torch.zeros(rows, 33, dtype=torch.bool)
    n_text = rows // 3
    t[:n_text, 32] = torch.randint(0, 1000, (n_text,), generator=g); m[:n_text, 32] = True
    t[n_text:, :32] = torch.randint(0, 2048, (rows - n_text, 32), generator=g); m[n_text:, :32] = True
    return t, m


def test_slot_refill_leaves_the_other_slots_bit_identical(tiny):
    """csm_prefill_slot (include/csm_hip.h; SURVEY.md 8b per-slot reset): B = 3 under greedy sampling; after 4 frames slot 1 is
    retired and re-prefilled with a NEW prompt of a different length while slots 0 and 2 keep generating.  Slots 0 and 2 must
    produce bit for bit the frames of an undisturbed run; the new utterance in slot 1 must produce bit for bit what it produces
    when it sits in slot 1 from the start (rows do not depend on their neighbours or on the global frame index)."""
    shape, w, m = tiny
    B, S = 3, 12
    pr = [_tiny_prompt(S, 50 + b) for b in range(B)]
    new_t, new_m = _tiny_prompt(9, 99)
    tok, msk = torch.stack([p[0] for p in pr]), torch.stack([p[1] for p in pr])

    def run(refill_at):
        m.reset_caches(); m.seed(11)
        m.prefill(tok, msk, torch.arange(S).unsqueeze(0).repeat(B, 1))
        m.depth(B, 1.0, 1, commit=True)
        f0 = None
        for k in range(1, 10):
            if k == refill_at:
                f0 = m.refill_slot(1, new_t, new_m, 1.0, 1).cpu()
            m.step(B, 1.0, 1)
        frames, eos = m.read_frames(B)
        return frames, f0

    und, _ = run(None)
    dis, f0 = run(4)
    assert und.shape == dis.shape == (10, B, 32)
    assert torch.equal(dis[:, 0], und[:, 0]) and torch.equal(dis[:, 2], und[:, 2]), "the refill disturbed a neighbouring slot"
    assert torch.equal(dis[:3, 1], und[:3, 1]) and torch.equal(dis[3, 1], f0), "history: the new utterance's frame 0 replaces the slot's newest entry"
    assert not torch.equal(dis[4:, 1], und[4:, 1])
    # the new utterance from the start of a batch that is filled slot by slot (prompts of different lengths)
    m.reset_caches(); m.seed(11)
    firsts = [m.refill_slot(b, *(pr[b] if b != 1 else (new_t, new_m)), 1.0, 1).cpu() for b in range(B)]
    assert m.num_frames() == 1
    for _ in range(6):
        m.step(B, 1.0, 1)
    ref, eos = m.read_frames(B)
    assert torch.equal(ref[0], torch.stack(firsts))
    assert torch.equal(firsts[1], f0) and torch.equal(ref[1:, 1], dis[4:, 1]), "the refilled utterance differs from the same utterance started with the batch"
    # (slot 0 here vs the rectangular prefill above: the same prompt, but frame 0 of a slot fill runs the batch-1 depth kernels and the
    #  rectangular one the batched ones -- different summation orders, so their greedy picks may part at a near-tie: not asserted)
    assert int(ref.min()) >= 0 and int(ref.max()) < 2051
    m.reset_slots([1])
    m.reset_caches()


def test_refill_beside_the_loop_leaves_the_other_slots_bit_identical_and_joins_in_the_batch(tiny):
    """csm_refill_begin / csm_refill_advance (include/csm_hip.h, round 4): B = 4, greedy; after 3 frames slot 2 is retired and its next
    prompt (another length) runs ONE backbone layer after each of the following frame steps while slots 0, 1, 3 keep generating; the step
    after the last layer samples the new utterance's frame 0 in the batch.  Slots 0, 1, 3: bit for bit the frames of an undisturbed
    run.  Slot 2 from its rejoin on: bit for bit the utterance it is when all four slots are filled this way before the first step
    (rows depend neither on their neighbours, nor on the global frame index, nor on how the prompt's layers were cut into calls)."""
    shape, w, m = tiny
    B, S = 4, 12
    pr = [_tiny_prompt(S, 60 + b) for b in range(B)]
    new_t, new_m = _tiny_prompt(9, 98)
    n_layers = m.bb.num_layers

    def fill(prompts, layers_per_call):
        m.reset_caches(); m.seed(11)
        for b, (t, mk) in enumerate(prompts):
            m.refill_begin(b, t, mk)
            while not m.refill_advance(layers_per_call):
                pass

    fill(pr, n_layers)
    for _ in range(12):
        m.step(B, 1.0, 1)
    und, _ = m.read_frames(B)
    fill(pr, n_layers)
    rejoin = None
    for k in range(12):
        m.step(B, 1.0, 1)
        if k == 2:
            m.refill_begin(2, new_t, new_m)
            with pytest.raises(RuntimeError, match="CSM_E_STATE"):
                m.refill_begin(1, new_t, new_m)                                   # one refill at a time
        if k >= 2 and rejoin is None and m.refill_advance(1):
            rejoin = m.num_frames()                                               # the next step's global index
    dis, eos = m.read_frames(B)
    assert rejoin == 2 + n_layers and und.shape == dis.shape == (12, B, 32)      # begun after frame 2, one layer per step from then on
    for b in (0, 1, 3):
        assert torch.equal(dis[:, b], und[:, b]), f"the refill disturbed slot {b}"
    assert torch.equal(dis[:3, 2], und[:3, 2]) and not torch.equal(dis[rejoin:, 2], und[rejoin:, 2])
    # the same utterance started with the batch, its prompt cut into calls differently
    fill([pr[0], pr[1], (new_t, new_m), pr[3]], 1 if n_layers > 1 else n_layers)
    for _ in range(12 - rejoin):
        m.step(B, 1.0, 1)
    ref, _ = m.read_frames(B)
    assert torch.equal(ref[:, 2], dis[rejoin:, 2]), "the utterance that joined a running batch differs from the same utterance started with the batch"
    assert torch.equal(ref[:, 0], und[: 12 - rejoin, 0])
    assert int(eos[2]) == -1 and int(dis.min()) >= 0 and int(dis.max()) < 2051
    m.reset_caches()


def test_csm1b_refill_beside_the_loop_at_batch_8(csm1b):
    """The same at CSM-1B size, B = 8 (batched persistent decoder, one-launch-free batched backbone chain, 16 layers): slot 5 is refilled with a
    60-row prompt four layers per frame step while the other seven keep generating under T = 0.9 / top-k 50 sampling -- their frames are bit
    for bit those of an undisturbed run (same seed: a frame step's noise depends on (seed, step, row) only), and the joined utterance's frames
    are those of the same utterance filled into slot 5 before the first step of a batch whose step counter is at the same value."""
    import bench
    from oracle import csm_ref as C
    from sesameai.models import Model, csm_1b_args
    gold, sd = csm1b
    B = 8
    tok, msk = bench.synthetic_prompt(_bench_args(), B + 1, C.csm_1b().text_vocab_size, seed0=8300)
    tok, msk = tok[:, :60], msk[:, :60]
    m = Model(csm_1b_args(), sd, max_frames=32, max_prefill_rows=B * 64)
    m.setup_caches(B)
    assert m.fast_paths() & 2

    def fill(rows):
        m.reset_caches(); m.seed(21)
        for b, r in enumerate(rows):
            m.refill_begin(b, tok[r], msk[r])
            while not m.refill_advance(16):
                pass

    fill(range(B))
    for _ in range(10):
        m.step(B, 0.9, 50)
    und, _ = m.read_frames(B)
    fill(range(B))
    rejoin = None
    for k in range(10):
        m.step(B, 0.9, 50)
        if k == 1:
            m.refill_begin(5, tok[B], msk[B])
        if k >= 1 and rejoin is None and m.refill_advance(4):
            rejoin = m.num_frames()
    dis, _ = m.read_frames(B)                                            # raises if a launch gave up
    assert rejoin == 5
    for b in range(B):
        if b != 5:
            assert torch.equal(dis[:, b], und[:, b]), f"the refill disturbed slot {b}"
    assert torch.equal(dis[:2, 5], und[:2, 5]) and int(dis.min()) >= 0 and int(dis.max()) < 2051
    # the greedy part of the claim (independent of the noise stream): the joined utterance's frame 0 is the batch's frame 0 of that prompt
    fill([0, 1, 2, 3, 4, B, 6, 7])
    m.step(B, 1.0, 1)
    ref0, _ = m.read_frames(B)
    fill(range(B))
    for k in range(2):
        m.step(B, 1.0, 1)
    m.refill_begin(5, tok[B], msk[B])
    while not m.refill_advance(5):
        pass
    m.step(B, 1.0, 1)
    got, _ = m.read_frames(B)
    assert torch.equal(got[2, 5], ref0[0, 5]), "frame 0 of the joined utterance differs from the same prompt's frame 0 at the start of a batch"
    m.reset_caches()


def test_continuous_batching_beside_the_loop_through_the_generator(tiny):
    """Generator.generate_codes_continuous with max_batch 4 takes the non-stalling path: 7 prompts of different lengths, 6 frames each,
    greedy -- every utterance equals the one the same prompt produces when it is filled into slot 0 of the same 4-slot batch alone."""
    from sesameai.generator import Generator
    shape, w, m = tiny
    gen = Generator.__new__(Generator)
    gen._model, gen._max_batch, gen._eos_poll, gen.device = m, 4, 4, m.device
    gen.refill_row_layers = 10                                                    # one layer of these short prompts per frame step
    prompts = [_tiny_prompt(6 + 2 * i, 400 + i) for i in range(7)]
    got = gen.generate_codes_continuous(prompts, 6, 1.0, 1)
    idle = _tiny_prompt(5, 7)
    for i, (t, mk) in enumerate(prompts):
        m.reset_caches()
        for b in range(4):
            m.refill_begin(b, *((t, mk) if b == 0 else idle))
            while not m.refill_advance(16):
                pass
        for _ in range(6):
            m.step(4, 1.0, 1)
        fr, _ = m.read_frames(4)
        assert got[i].shape == (6, 32) and torch.equal(got[i], fr[:, 0]), f"utterance {i}"
    m.reset_caches()


def test_refill_gates_share_one_predicate_and_a_parked_slot_holds_its_position(monkeypatch):
    """ADVICE r4 (medium + low).  csm_refill_begin, the frame step's inject node, k_advance's use of the slots' flags and the host's
    choice of the refill path now share ONE predicate (csm_refill_supported): with CSM_WIDE_MIN above the running batch a frame step used
    to consume the fresh flag without ever injecting the prompt's last row (frame 0 silently sampled from the placeholder), and with
    CSM_WIDE=0 iter_codes_continuous raised instead of falling back to csm_prefill_slot.  A parked slot's position is HELD while its prompt
    runs (it used to advance every step and could trip the sticky overflow flag for the whole batch); csm_reset_slots / csm_prefill_slot on
    the slot whose refill is running are refused."""
    from sesameai.generator import Generator
    from sesameai.models import Model, csm_tiny_args, synthetic_state_dict
    sd = synthetic_state_dict(csm_tiny_args(), seed=1234)
    monkeypatch.setenv("CSM_WIDE_MIN", "4")
    m = Model(csm_tiny_args(), sd, max_frames=64, max_prefill_rows=256)
    m.setup_caches(4)
    assert m.supports_refill_beside_the_loop() and m.supports_refill_beside_the_loop(4) and not m.supports_refill_beside_the_loop(3)
    pr = [_tiny_prompt(12, 70 + b) for b in range(4)]
    new_t, new_m = _tiny_prompt(9, 97)

    def fill(prompts):
        m.reset_caches(); m.seed(3)
        for b, (t, mk) in enumerate(prompts):
            m.refill_begin(b, t, mk)
            while not m.refill_advance(16):
                pass
    fill([pr[0], (new_t, new_m), pr[2], pr[3]])
    with pytest.raises(RuntimeError, match="CSM_E_STATE"):
        m.step(3, 1.0, 1)                                     # three rows take the GEMV path here: the fresh slots would be stepped as they are
    m.step(4, 1.0, 1)
    want0 = m.read_frames(4)[0][0, 1]                         # the new utterance's frame 0 when it starts with the batch
    fill(pr)
    m.step(4, 1.0, 1)
    m.refill_begin(1, new_t, new_m)
    with pytest.raises(RuntimeError, match="CSM_E_STATE"):
        m.step(3, 1.0, 1)
    with pytest.raises(RuntimeError, match="CSM_E_STATE"):
        m.reset_slots([1])
    with pytest.raises(RuntimeError, match="CSM_E_STATE"):
        m.refill_slot(1, new_t, new_m, 1.0, 1)
    for k in range(300):                                      # 9 + 300 > max_seq_len = 256: the parked position must not move
        m.step(4, 1.0, 1)
        if k % 100 == 99:
            m.reset_slots([0, 2, 3])                          # (the generating slots would run out of positions themselves)
    m.read_frames(4, m.num_frames() - 1, 1)                   # CSM_E_TOO_LONG here before the fix
    while not m.refill_advance(1):
        m.step(4, 1.0, 1)
    m.step(4, 1.0, 1)
    got0 = m.read_frames(4, m.num_frames() - 1, 1)[0][0, 1]
    assert torch.equal(got0, want0), "the joined utterance's frame 0 differs from the same prompt's frame 0 at the start of a batch"
    # a batch the predicate rules out takes the csm_prefill_slot path by itself
    gen = Generator.__new__(Generator)
    gen._model, gen._max_batch, gen._eos_poll, gen.device = m, 3, 4, m.device
    prompts = [_tiny_prompt(6 + 2 * i, 500 + i) for i in range(5)]
    got = gen.generate_codes_continuous(prompts, 5, 1.0, 1)
    assert all(g.shape == (5, 32) for g in got)
    del m
    monkeypatch.setenv("CSM_WIDE", "0")
    m2 = Model(csm_tiny_args(), sd, max_frames=64, max_prefill_rows=256)
    m2.setup_caches(4)
    assert not m2.supports_refill_beside_the_loop()
    with pytest.raises(RuntimeError, match="CSM_E_STATE"):
        m2.refill_begin(0, new_t, new_m)
    gen._model, gen._max_batch = m2, 4
    got2 = gen.generate_codes_continuous(prompts, 5, 1.0, 1)     # raised CSM_E_STATE before the fix
    assert all(g.shape == (5, 32) for g in got2)


def test_slot_refills_draw_from_their_own_noise_streams(tiny):
    """under stochastic sampling every slot refilled between the same two frame steps drew frame 0 from the SAME
    Philox stream (step counter not advanced, sequence index 0), so N copies of one prompt started with identical frames, and slot 0's
    frame 0 shared its draws with slot 0's next frame.  Refills now draw from a second key domain with a per-refill counter
    (csm_seed, include/csm_hip.h).  Same prompt into three slots at T = 0.9 / top-k 50: three different frame 0s, still a pure
    function of the seed; the frame steps that follow are untouched by HOW MANY refills happened before them (their own counter)."""
    shape, w, m = tiny
    t, mk = _tiny_prompt(12, 123)
    T, K = 0.9, 50

    def fill(seed, n_extra=0):
        m.reset_caches(); m.seed(seed)
        f0 = [m.refill_slot(b, t, mk, T, K).cpu() for b in range(3)]
        for _ in range(n_extra):                                             # refill slot 2 again and again: only ITS frame 0 changes
            f0[2] = m.refill_slot(2, t, mk, T, K).cpu()
        assert torch.equal(m.last_frame(3).cpu(), torch.stack(f0)), "csm_copy_frame must keep returning every slot's own newest frame"
        for _ in range(3):
            m.step(3, T, K)
        fr, _ = m.read_frames(3)
        return torch.stack(f0), fr

    f0, fr = fill(5)
    assert not torch.equal(f0[0], f0[1]) and not torch.equal(f0[1], f0[2]) and not torch.equal(f0[0], f0[2]), "identical frame 0 in different slots"
    assert int((f0[0] == f0[1]).sum()) < 16, "the slots' draws are correlated"
    assert not torch.equal(fr[0, 0], fr[1, 0]), "slot 0: frame 0 and frame 1 drawn alike"
    f0b, frb = fill(5)
    assert torch.equal(f0, f0b) and torch.equal(fr, frb), "sampling is a pure function of the seed"
    f0c, frc = fill(6)
    assert not torch.equal(f0, f0c)
    f0d, frd = fill(5, n_extra=2)
    assert torch.equal(f0d[:2], f0[:2]) and not torch.equal(f0d[2], f0[2])
    assert torch.equal(frd[1:, :2], fr[1:, :2]), "frame steps of the undisturbed slots depend on the number of refills before them"
    m.reset_caches()


def test_continuous_batching_through_the_generator_matches_one_utterance_at_a_time(tiny):
    """Generator.generate_codes_continuous on the device: 5 prompts of different lengths through 2 slots, 6 frames each (greedy;
    random weights never emit the EOS frame, so utterances retire at the length limit) -- every utterance must equal the one the
    same prompt produces when it is the only one refilled into slot 0 of the same 2-slot batch."""
    from sesameai.generator import Generator
    shape, w, m = tiny
    gen = Generator.__new__(Generator)
    gen._model, gen._max_batch, gen._eos_poll, gen.device = m, 2, 4, m.device
    prompts = [_tiny_prompt(6 + 3 * i, 200 + i) for i in range(5)]
    got = gen.generate_codes_continuous(prompts, 6, 1.0, 1)
    idle = _tiny_prompt(5, 7)
    for i, (t, mk) in enumerate(prompts):
        m.reset_caches()
        f0 = m.refill_slot(0, t, mk, 1.0, 1).cpu()
        m.refill_slot(1, *idle, 1.0, 1)
        for _ in range(5):
            m.step(2, 1.0, 1)
        fr, _ = m.read_frames(2)
        want = torch.cat([f0.unsqueeze(0), fr[1:, 0]])
        assert got[i].shape == (6, 32) and torch.equal(got[i], want), f"utterance {i}"
    m.reset_caches()


def test_positions_beyond_max_seq_are_reported_not_clamped(tiny):
    """pos >= max_seq used to be clamped silently inside the kernels.  Host-visible positions raise at once;
    positions that only exist on the device raise CSM_E_TOO_LONG at the next read_frames."""
    shape, w, m = tiny                     # tiny backbone: max_seq_len 256
    tok = torch.zeros(1, 4, 33, dtype=torch.long); msk = torch.zeros(1, 4, 33, dtype=torch.bool); msk[:, :, 32] = True
    with pytest.raises(ValueError, match="input_pos outside"):
        m.prefill(tok, msk, torch.tensor([[253, 254, 255, 256]]))
    m.reset_caches()
    m.prefill(tok, msk, torch.tensor([[250, 251, 252, 253]]))
    m.depth(1, 1.0, 1, commit=True)
    for _ in range(2):                     # positions 254, 255: still inside
        m.step(1, 1.0, 1)
    frames, eos = m.read_frames(1)
    assert frames.shape[0] == 3
    m.step(1, 1.0, 1)                      # position 256: outside
    with pytest.raises(RuntimeError, match="CSM_E_TOO_LONG"):
        m.read_frames(1)
    m.reset_caches()                       # the flag is part of the per-utterance state
    m.prefill(tok, msk, torch.tensor([[0, 1, 2, 3]]))
    m.depth(1, 1.0, 1, commit=True)
    assert m.read_frames(1)[0].shape[0] == 1


# ----------------------------------------------------------------------------------------
# BASELINE configs 2, 3 and 5 at their stated size against goldens of the oracle (oracle/make_golden.py cfg2/cfg3/cfg5)
# ----------------------------------------------------------------------------------------
def _bench_args():
    from types import SimpleNamespace
    return SimpleNamespace(ctx_text=40, ctx_frames=125, gen_text=24)


def _same_until_a_near_tie(got, want, margin, noise, what, tie=NEAR_TIE):
    """A free-running greedy frame (each codebook conditioned on the codes picked before it): identical to the oracle's
    up to the first difference, and that difference must sit where the ORACLE's top-1/top-2 margin is inside the
    rounding-noise floor.  Returns the number of decisions that were compared (= matched)."""
    want = want.to(got.dtype)
    diff = (got != want).nonzero().flatten()
    if diff.numel() == 0:
        return int(got.numel())
    first = int(diff[0])
    _excuse(float(margin[first]), noise, f"{what}: codebook {first} differs", tie=tie)
    return first


def _teacher_forced(m, gold, S, n_frames, noise, what, tie=NEAR_TIE, max_excused=0.08):
    """depth() on the current backbone state for golden frames 0..n-1, feeding the golden codes back one row at a time."""
    max_diff, mism = 0.0, []
    for f in range(n_frames):
        forced = gold["codes"][f].reshape(1, -1)
        out, logits = m.depth(1, 1.0, 1, forced=forced, want_logits=True, commit=False)
        lg = logits[:, 0].float().cpu()
        max_diff = max(max_diff, (torch.gather(lg, 1, gold["top_i"][f].long()) - gold["top_v"][f].float()).abs().max().item())
        for cb in (out[0].cpu() != gold["codes"][f].reshape(-1)).nonzero().flatten().tolist():
            mism.append((f, cb, float(gold["margin"][f, cb])))
        if f + 1 < n_frames:
            row = torch.zeros(1, 1, 33, dtype=torch.long); row[0, 0, :32] = gold["codes"][f].reshape(-1).long()
            rmask = torch.ones(1, 1, 33, dtype=torch.bool); rmask[0, 0, 32] = False
            m.prefill(row, rmask, torch.tensor([[S + f]]))
    print(f"{what}: max|dlogit|={max_diff:.4f} (oracle bf16-vs-fp32 gap {noise:.4f}); {len(mism)} of {32 * n_frames} greedy rows excused as near-ties "
          f"({100.0 * len(mism) / (32 * n_frames):.1f} %): {mism}")
    assert max_diff <= noise, what
    assert len(mism) <= max(max_excused * 32 * n_frames, 3), f"{what}: too many greedy rows differ from the oracle, near-ties or not" 
    for f, cb, margin in mism:
        _excuse(margin, noise, f"{what}: greedy index differs at frame {f} codebook {cb}", tie=tie)
    return max_diff


def test_csm1b_config2_prompt_vs_golden(csm1b):
    """BASELINE config 2 = the bench workload: S = 190 prompt rows WITH audio rows (40 text + 125 audio + EOS + 24 text),
    through both prefill forms (Generator's prompt mode and bench.py's plain csm_prefill), 6 frames."""
    import bench
    from oracle import csm_ref as C
    from sesameai.models import Model, csm_1b_args
    _, sd = csm1b
    gold = torch.load(os.path.join(GOLD, "csm1b_cfg2.pt"))
    tok, msk = gold["prompt_tokens"], gold["prompt_mask"]
    bt, bm = bench.synthetic_prompt(_bench_args(), 1, C.csm_1b().text_vocab_size, seed0=2025)
    assert torch.equal(bt[0], tok) and torch.equal(bm[0], msk), "golden prompt is not bench.py's config-2 prompt"
    S = tok.shape[0]
    assert S == 190
    noise = float(gold["bf16_vs_fp32_gap"].max())
    m = Model(csm_1b_args(), sd, max_frames=64, max_prefill_rows=256)
    m.setup_caches(1)
    m.prefill_prompt(tok.unsqueeze(0), msk.unsqueeze(0))
    _teacher_forced(m, gold, S, gold["codes"].shape[0], noise, "config 2, prompt-mode prefill")
    m.reset_caches()
    m.prefill(tok.unsqueeze(0), msk.unsqueeze(0), torch.arange(S).unsqueeze(0))
    _teacher_forced(m, gold, S, 2, noise, "config 2, plain prefill (bench.py)")
    # the replayed hipGraph frame step from the golden state: greedy codes equal the oracle's up to the first near-tie
    m.reset_caches()
    m.prefill(tok.unsqueeze(0), msk.unsqueeze(0), torch.arange(S).unsqueeze(0))
    m.depth(1, 1.0, 1, forced=gold["codes"][0].reshape(1, -1), commit=True)
    n_cmp = 0
    for f in range(1, gold["codes"].shape[0]):
        row = torch.zeros(1, 1, 33, dtype=torch.long); row[0, 0, :32] = gold["codes"][f - 1].reshape(-1).long()
        rmask = torch.ones(1, 1, 33, dtype=torch.bool); rmask[0, 0, 32] = False
        got = m.generate_frame(row, rmask, torch.tensor([[S + f - 1]]), 1.0, 1)[0].cpu()
        n_cmp += _same_until_a_near_tie(got, gold["codes"][f].reshape(-1), gold["margin"][f], noise, f"graph step, frame {f}")
    assert n_cmp >= 32, "too few comparable greedy decisions"


def test_csm1b_config3_batch32_vs_golden(csm1b):
    """BASELINE config 3: B = 32 x the config-2 shape.  Teacher-forced logits of every utterance against the BATCHED
    oracle (the >= 24-row operand-order decode path included -- vs the oracle, not vs itself), then a hipGraph-replayed
    frame step whose greedy codes must equal the oracle's up to each utterance's first near-tie."""
    import bench
    from oracle import csm_ref as C
    from sesameai.models import Model, csm_1b_args
    _, sd = csm1b
    gold = torch.load(os.path.join(GOLD, "csm1b_cfg3.pt"))
    # the oracle's bf16-vs-fp32 gap ON THESE 2,048 ROWS (oracle/make_golden.py cfg3gap, round 4: 0.143 / 0.124 for the two frames).  Rounds 2-3
    # used config 2's gap (0.1135: a maximum over 192 rows of one utterance) and needed 1.1x; tools/dbg/bisect_b32_gap.sh showed HIP's maximum
    # move between 0.094 and 0.125 with the fp32 summation order of the prefill alone (profiles/r04/bisect_b32_gap.txt) -- a maximum over ten
    # times the samples, not an op that is off.  Near-ties are still judged against config 2's gap (the margins are per row).
    noise32 = float(gold["bf16_vs_fp32_gap"].max())
    g2 = torch.load(os.path.join(GOLD, "csm1b_cfg2.pt"))
    noise = float(g2["bf16_vs_fp32_gap"].max())
    tok, msk = gold["prompt_tokens"].long(), gold["prompt_mask"]
    B, S = tok.shape[0], tok.shape[1]
    assert (B, S) == (32, 190)
    bt, bm = bench.synthetic_prompt(_bench_args(), B, C.csm_1b().text_vocab_size, seed0=2025)
    assert torch.equal(bt, tok) and torch.equal(bm, msk)
    m = Model(csm_1b_args(), sd, max_frames=16, max_prefill_rows=B * S)
    m.setup_caches(B)
    m.prefill(tok, msk, torch.arange(S).unsqueeze(0).repeat(B, 1))
    codes0 = gold["codes"][0]                                                     # [B][32]
    out, logits = m.depth(B, 1.0, 1, forced=codes0, want_logits=True, commit=True)    # logits [32][B][V]
    lg = logits.float().cpu()
    d0 = (torch.gather(lg, 2, gold["top_i"][0].long()) - gold["top_v"][0].float()).abs().max().item()
    bad = (out.cpu() != codes0).nonzero()
    for b, cb in bad.tolist():
        _excuse(float(gold["margin"][0][cb, b]), noise, f"frame 0 utterance {b} codebook {cb}", tie=BATCH32_TIE)
    # frame 1: graph replay on the golden inputs (decode-step kernels at M = 32 rows, operand-order activations)
    row = torch.zeros(B, 1, 33, dtype=torch.long); row[:, 0, :32] = codes0.long()
    rmask = torch.ones(B, 1, 33, dtype=torch.bool); rmask[:, 0, 32] = False
    got = m.generate_frame(row, rmask, torch.full((B, 1), S), 1.0, 1).cpu()
    n_cmp = 0
    for b in range(B):
        n_cmp += _same_until_a_near_tie(got[b], gold["codes"][1][b], gold["margin"][1][:, b], noise, f"graph step, utterance {b}", tie=BATCH32_TIE)
    # and its logits, teacher-forced, through the same decode-step kernels
    m2 = Model(csm_1b_args(), sd, max_frames=16, max_prefill_rows=B * S)
    m2.setup_caches(B)
    m2.prefill(tok, msk, torch.arange(S).unsqueeze(0).repeat(B, 1))
    m2.prefill(row, rmask, torch.full((B, 1), S))
    out1, logits1 = m2.depth(B, 1.0, 1, forced=gold["codes"][1], want_logits=True, commit=False)
    d1 = (torch.gather(logits1.float().cpu(), 2, gold["top_i"][1].long()) - gold["top_v"][1].float()).abs().max().item()
    print(f"config 3 (B=32): max|dlogit| frame 0 {d0:.4f}, frame 1 {d1:.4f} (the oracle's gap on these rows {noise32:.4f}, on config 2's {noise:.4f}); {len(bad)} of {B * 32} greedy rows excused as near-ties "
          f"({100.0 * len(bad) / (B * 32):.1f} %); {n_cmp} of {B * 32} graph-step decisions compared")
    assert max(d0, d1) <= noise32                # 1x, like B = 1 and B = 4 (measured 0.82x)
    assert len(bad) <= 0.08 * B * 32
    assert n_cmp >= B * 8


def test_csm1b_config5_fp8_long_context_vs_golden(csm1b):
    """BASELINE config 5 in its stated form: fp8-e4m3 weight stream, S = 1334 prompt rows (10 segments) and positions
    ~1700 (KV stream 55 MB per step), against the oracle running on the dequantised weights."""
    from sesameai.models import Model, csm_1b_args
    _, sd = csm1b
    gold = torch.load(os.path.join(GOLD, "csm1b_cfg5.pt"))
    m = Model(csm_1b_args(), sd, max_frames=16, max_prefill_rows=1700, weights_dtype="fp8")
    got = torch.stack([m._w["backbone.layers.3.mlp.w2.weight"].float().abs().sum(), m._w["decoder.layers.1.attn.q_proj.weight"].float().abs().sum(),
                       m._w["audio_head"].float().abs().sum()]).cpu()
    assert torch.allclose(got, gold["deq_checksum"], rtol=1e-4), "product and oracle fp8 dequantisation differ"
    m.setup_caches(1)
    assert m.fast_paths() & 16, "fp8 mode must run the backbone as the one-launch layer on the e4m3 stream (k_bb_layer<true>)"
    assert m.fast_paths() & 1, "fp8 mode must run the persistent depth decoder"
    for key, S_want in (("s1334", 1334), ("s1700", 1700)):
        g = gold[key]
        tok, msk = g["prompt_tokens"].long(), g["prompt_mask"]
        S = tok.shape[0]
        assert S == S_want
        noise = float(g["bf16_vs_fp32_gap"].max())
        m.reset_caches()
        m.prefill_prompt(tok.unsqueeze(0), msk.unsqueeze(0))
        _teacher_forced(m, g, S, 2, noise, f"config 5 fp8, S={S}")
        # replayed graph step at position S (fp8 GEMV stream, split-K attention over S+1 keys)
        m.reset_caches()
        m.prefill_prompt(tok.unsqueeze(0), msk.unsqueeze(0))
        m.depth(1, 1.0, 1, forced=g["codes"][0].reshape(1, -1), commit=True)
        row = torch.zeros(1, 1, 33, dtype=torch.long); row[0, 0, :32] = g["codes"][0].reshape(-1).long()
        rmask = torch.ones(1, 1, 33, dtype=torch.bool); rmask[0, 0, 32] = False
        got1 = m.generate_frame(row, rmask, torch.tensor([[S]]), 1.0, 1)[0].cpu()
        assert _same_until_a_near_tie(got1, g["codes"][1].reshape(-1), g["margin"][1], noise, f"graph step at p={S}") >= 1


def test_csm1b_config5_batched_fp8_long_context_vs_golden(csm1b):
    """BASELINE config 5, batched (SURVEY.md 8d lists B = 32 for it; the fixture keeps B = 4): four DIFFERENT 1334-row prompts, fp8-e4m3
    weight stream, against the BATCHED oracle on the dequantised weights -- the LDS-tiled prefill at 5,336 rows, the batched
    decode step's split-K attention over 1,335 keys per row, the e4m3 matrix-core path and the batched persistent decoder."""
    import bench
    from types import SimpleNamespace
    from oracle import csm_ref as C
    from sesameai.models import Model, csm_1b_args
    _, sd = csm1b
    path = os.path.join(GOLD, "csm1b_cfg5b.pt")
    if not os.path.exists(path):
        pytest.skip("csm1b_cfg5b golden not generated (oracle/make_golden.py --only cfg5b)")
    gold = torch.load(path)
    g5 = torch.load(os.path.join(GOLD, "csm1b_cfg5.pt"))
    noise = float(g5["s1334"]["bf16_vs_fp32_gap"].max())
    tok, msk = gold["prompt_tokens"].long(), gold["prompt_mask"]
    B, S = tok.shape[0], tok.shape[1]
    assert (B, S) == (4, 1334)
    bt, bm = bench.synthetic_prompt(SimpleNamespace(ctx_text=30, ctx_frames=100, gen_text=24), B, C.csm_1b().text_vocab_size, seed0=6000,
                                    segments=10, ctx_text=30, ctx_frames=100)
    assert torch.equal(bt, tok) and torch.equal(bm, msk), "golden prompts are not bench.py's config-5 prompts"
    m = Model(csm_1b_args(), sd, max_frames=16, max_prefill_rows=B * S, weights_dtype="fp8")
    m.setup_caches(B)
    assert m.fast_paths() & 2, "the batched persistent decoder must be on this path"
    m.prefill(tok, msk, torch.arange(S).unsqueeze(0).repeat(B, 1))
    codes0 = gold["codes"][0]
    out, logits = m.depth(B, 1.0, 1, forced=codes0, want_logits=True, commit=True)
    d0 = (torch.gather(logits.float().cpu(), 2, gold["top_i"][0].long()) - gold["top_v"][0].float()).abs().max().item()
    bad = (out.cpu() != codes0).nonzero()
    for b, cb in bad.tolist():
        _excuse(float(gold["margin"][0][cb, b]), noise, f"frame 0 utterance {b} codebook {cb}", tie=BATCH32_TIE)
    row = torch.zeros(B, 1, 33, dtype=torch.long); row[:, 0, :32] = codes0.long()
    rmask = torch.ones(B, 1, 33, dtype=torch.bool); rmask[:, 0, 32] = False
    got = m.generate_frame(row, rmask, torch.full((B, 1), S), 1.0, 1).cpu()
    n_cmp = sum(_same_until_a_near_tie(got[b], gold["codes"][1][b], gold["margin"][1][:, b], noise, f"graph step, utterance {b}", tie=BATCH32_TIE) for b in range(B))
    m2 = Model(csm_1b_args(), sd, max_frames=16, max_prefill_rows=B * S, weights_dtype="fp8")
    m2.setup_caches(B)
    m2.prefill(tok, msk, torch.arange(S).unsqueeze(0).repeat(B, 1))
    m2.prefill(row, rmask, torch.full((B, 1), S))
    out1, logits1 = m2.depth(B, 1.0, 1, forced=gold["codes"][1], want_logits=True, commit=False)
    d1 = (torch.gather(logits1.float().cpu(), 2, gold["top_i"][1].long()) - gold["top_v"][1].float()).abs().max().item()
    print(f"config 5 batched (B=4, S=1334, fp8): max|dlogit| frame 0 {d0:.4f}, frame 1 {d1:.4f} (gap {noise:.4f}); {len(bad)} of {B * 32} greedy rows excused; "
          f"{n_cmp} of {B * 32} graph-step decisions compared")
    assert max(d0, d1) <= noise
    assert len(bad) <= 0.08 * B * 32 + 1 and n_cmp >= B * 4


def test_csm1b_config5_batch32_fp8_long_context_vs_golden(csm1b):
    """BASELINE config 5 at the batch SURVEY.md 8d names for it: B = 32 x the 1334-row prompt (bench.py's `config5_b32` leg, seeds
    6000..6031), fp8-e4m3 weight stream, against the BATCHED oracle on the dequantised weights (tests/golden/csm1b_cfg5c.pt: top-8
    logits, codes and margins of 2 teacher-forced frames; the prompts are rebuilt from the seeds and checked by checksum).  Covers
    the LDS-tiled prefill at 42,688 rows, the 32-row e4m3 matrix-core decode step with split-key attention over 1,335 keys per row
    and the batched persistent decoder (k_dec_persist_m<2>)."""
    import bench
    from types import SimpleNamespace
    from oracle import csm_ref as C
    from sesameai.models import Model, csm_1b_args
    _, sd = csm1b
    path = os.path.join(GOLD, "csm1b_cfg5c.pt")
    if not os.path.exists(path):
        pytest.skip("csm1b_cfg5c golden not generated (oracle/make_golden.py --only cfg5c)")
    gold = torch.load(path)
    g5 = torch.load(os.path.join(GOLD, "csm1b_cfg5.pt"))
    noise = float(g5["s1334"]["bf16_vs_fp32_gap"].max())                    # per-row near-tie scale (one utterance)
    noise32 = float(gold["bf16_vs_fp32_gap"].max()) if "bf16_vs_fp32_gap" in gold else 1.1 * noise      # the oracle's gap on THESE 2,048 rows (make_golden cfg5cgap)
    B, S = 32, 1334
    tok, msk = bench.synthetic_prompt(SimpleNamespace(ctx_text=30, ctx_frames=100, gen_text=24), B, C.csm_1b().text_vocab_size, seed0=int(gold["prompt_seed"]),
                                      segments=10, ctx_text=30, ctx_frames=100)
    assert tok.shape == (B, S, 33) and torch.equal(tok.sum(dim=(1, 2)), gold["prompt_checksum"]), "these are not the golden's prompts"
    m = Model(csm_1b_args(), sd, max_frames=16, max_prefill_rows=B * S, weights_dtype="fp8")
    m.setup_caches(B)
    assert m.fast_paths() & 2, "the batched persistent decoder must be on this path"
    m.prefill(tok, msk, torch.arange(S).unsqueeze(0).repeat(B, 1))
    codes0 = gold["codes"][0]
    out, logits = m.depth(B, 1.0, 1, forced=codes0, want_logits=True, commit=True)
    d0 = (torch.gather(logits.float().cpu(), 2, gold["top_i"][0].long()) - gold["top_v"][0].float()).abs().max().item()
    bad = (out.cpu() != codes0).nonzero()
    for b, cb in bad.tolist():
        _excuse(float(gold["margin"][0][cb, b]), noise, f"frame 0 utterance {b} codebook {cb}", tie=BATCH32_TIE)
    row = torch.zeros(B, 1, 33, dtype=torch.long); row[:, 0, :32] = codes0.long()
    rmask = torch.ones(B, 1, 33, dtype=torch.bool); rmask[:, 0, 32] = False
    got = m.generate_frame(row, rmask, torch.full((B, 1), S), 1.0, 1).cpu()
    n_cmp = sum(_same_until_a_near_tie(got[b], gold["codes"][1][b], gold["margin"][1][:, b], noise, f"graph step, utterance {b}", tie=BATCH32_TIE) for b in range(B))
    del m
    m2 = Model(csm_1b_args(), sd, max_frames=16, max_prefill_rows=B * S, weights_dtype="fp8")
    m2.setup_caches(B)
    m2.prefill(tok, msk, torch.arange(S).unsqueeze(0).repeat(B, 1))
    m2.prefill(row, rmask, torch.full((B, 1), S))
    out1, logits1 = m2.depth(B, 1.0, 1, forced=gold["codes"][1], want_logits=True, commit=False)
    d1 = (torch.gather(logits1.float().cpu(), 2, gold["top_i"][1].long()) - gold["top_v"][1].float()).abs().max().item()
    print(f"config 5 at B=32 (S=1334, fp8): max|dlogit| frame 0 {d0:.4f}, frame 1 {d1:.4f} (the oracle's gap on these rows {noise32:.4f}, on one utterance {noise:.4f}); {len(bad)} of {B * 32} greedy rows excused; "
          f"{n_cmp} of {B * 32} graph-step decisions compared")
    assert max(d0, d1) <= noise32
    assert len(bad) <= 0.08 * B * 32 and n_cmp >= B * 8


def test_csm1b_config4_one_shard_vs_golden(csm1b):
    """BASELINE config 4 = batch 256 sharded over 8 GPUs, 32 utterances per rank, no per-step collective: rank r runs bench.py's prompts of seeds
    4000 + 32 r .. (`batch32_leg`).  No 8-GPU node has been available to this build (the N > 1 control flow is rehearsed in
    tests/test_bench_contract_gpu.py); what one GPU CAN show is that a shard computes what the batched oracle computes for ITS prompts --
    here the last rank's, seeds 4224..4255 (tests/golden/csm1b_cfg4_rank7.pt: top-8 logits, codes, margins of 2 teacher-forced frames, the
    oracle's bf16-vs-fp32 gap on those 2,048 rows): prefill of 32 x 190 rows, frame 0, the replayed graph step."""
    import bench
    from oracle import csm_ref as C
    from sesameai.models import Model, csm_1b_args
    _, sd = csm1b
    path = os.path.join(GOLD, "csm1b_cfg4_rank7.pt")
    if not os.path.exists(path):
        pytest.skip("csm1b_cfg4_rank7 golden not generated (oracle/make_golden.py --only cfg4)")
    gold = torch.load(path)
    g2 = torch.load(os.path.join(GOLD, "csm1b_cfg2.pt"))
    noise = float(g2["bf16_vs_fp32_gap"].max())                         # per-row near-tie scale (one utterance)
    noise32 = float(gold["bf16_vs_fp32_gap"].max())                     # the oracle's gap on THESE 2,048 rows
    B = 32
    assert int(gold["prompt_seed"]) == 4000 + 32 * int(gold["rank"])
    tok, msk = bench.synthetic_prompt(_bench_args(), B, C.csm_1b().text_vocab_size, seed0=int(gold["prompt_seed"]))
    S = tok.shape[1]
    assert S == 190 and torch.equal(tok.sum(dim=(1, 2)), gold["prompt_checksum"]), "these are not the golden's prompts"
    m = Model(csm_1b_args(), sd, max_frames=16, max_prefill_rows=B * S)
    m.setup_caches(B)
    assert m.fast_paths() & 2, "the batched persistent decoder must be on this path"
    m.prefill(tok, msk, torch.arange(S).unsqueeze(0).repeat(B, 1))
    codes0 = gold["codes"][0]
    out, logits = m.depth(B, 1.0, 1, forced=codes0, want_logits=True, commit=True)
    d0 = (torch.gather(logits.float().cpu(), 2, gold["top_i"][0].long()) - gold["top_v"][0].float()).abs().max().item()
    bad = (out.cpu() != codes0).nonzero()
    for b, cb in bad.tolist():
        _excuse(float(gold["margin"][0][cb, b]), noise, f"frame 0 utterance {b} codebook {cb}", tie=BATCH32_TIE)
    row = torch.zeros(B, 1, 33, dtype=torch.long); row[:, 0, :32] = codes0.long()
    rmask = torch.ones(B, 1, 33, dtype=torch.bool); rmask[:, 0, 32] = False
    got = m.generate_frame(row, rmask, torch.full((B, 1), S), 1.0, 1).cpu()
    n_cmp = sum(_same_until_a_near_tie(got[b], gold["codes"][1][b], gold["margin"][1][:, b], noise, f"graph step, utterance {b}", tie=BATCH32_TIE) for b in range(B))
    del m
    m2 = Model(csm_1b_args(), sd, max_frames=16, max_prefill_rows=B * S)
    m2.setup_caches(B)
    m2.prefill(tok, msk, torch.arange(S).unsqueeze(0).repeat(B, 1))
    m2.prefill(row, rmask, torch.full((B, 1), S))
    out1, logits1 = m2.depth(B, 1.0, 1, forced=gold["codes"][1], want_logits=True, commit=False)
    d1 = (torch.gather(logits1.float().cpu(), 2, gold["top_i"][1].long()) - gold["top_v"][1].float()).abs().max().item()
    print(f"config 4, rank {int(gold['rank'])}'s shard (B=32, seeds {int(gold['prompt_seed'])}..): max|dlogit| frame 0 {d0:.4f}, frame 1 {d1:.4f} (the oracle's gap on these rows "
          f"{noise32:.4f}); {len(bad)} of {B * 32} greedy rows excused; {n_cmp} of {B * 32} graph-step decisions compared")
    assert max(d0, d1) <= noise32
    assert len(bad) <= 0.08 * B * 32 and n_cmp >= B * 8


def test_csm1b_prompt_to_pcm_composed_on_the_bench_checkpoint(csm1b):
    """The composed path on the N(0, 0.02^2) BENCH checkpoint: BASELINE config 2's prompt given as the reference gives it (a voice-prompt
    Segment + the text to speak) -> Generator.generate (prompt assembly, prefill, hipGraph frame loop, Mimi decode on the GPU), greedy, 10
    frames, against csm_ref run live on this host.  What this checkpoint can carry: the prompt assembly is the golden prompt's; the frame in
    which the free-running trajectories part parts at a codebook where the oracle's margin is inside NEAR_TIE x gap (with near-uniform logits
    23 % of the oracle's rows are such near-ties, so they part within a frame or two); and generate()'s samples are mimi_ref's decode of the
    codes the frame loop produced (2e-5 x peak).  The statement north_star makes -- codes bit-exact under greedy and PCM within tolerance of
    the reference pipeline, over whole clips -- is tested on the DECISIVE checkpoint: tests/test_decisive_gpu.py (64 frames, zero excused rows).
    (Round 4's version also compared PCM 'over the frames identical to the oracle's' -- zero frames on this checkpoint, a vacuous branch: gone.)"""
    from oracle import csm_ref as C, mimi_ref as M
    from sesameai.generator import Generator, Segment
    from sesameai.mimi import MimiArgs, MimiCodec, synthetic_state_dict as mimi_sd
    from sesameai.models import Model, csm_1b_args
    _, sd = csm1b
    g2 = torch.load(os.path.join(GOLD, "csm1b_cfg2.pt"))
    noise = float(g2["bf16_vs_fp32_gap"].max())
    tok, msk = g2["prompt_tokens"], g2["prompt_mask"]                      # = bench.py's config-2 prompt (asserted in the config-2 test)
    n_frames = 10
    ctx = [Segment(speaker=1, text=tok[:40, 32].tolist(), audio_codes=tok[40:165, :32].t().contiguous())]
    text = tok[166:, 32].tolist()
    model = Model(csm_1b_args(), sd, max_frames=32, max_prefill_rows=256)
    codec = MimiCodec(MimiArgs(), mimi_sd(MimiArgs(), seed=4321), max_frames=32)
    gen = Generator(model, audio_tokenizer=codec)
    pt, pm = gen._build_prompt(text, 1, ctx)
    assert torch.equal(pt.cpu(), tok) and torch.equal(pm.cpu(), msk), "prompt assembly differs from the golden prompt"
    frames = gen.generate_codes(pt, pm, n_frames, 1.0, 1)[:, 0]            # [n][32] -- what generate() decodes
    pcm = gen.generate(text, 1, ctx, max_audio_length_ms=n_frames * 80, temperature=1.0, topk=1).cpu()
    assert pcm.shape == (n_frames * 1920,)
    shape = C.csm_1b()
    om = C.OracleModel(shape, C.make_weights(shape, seed=1234)); om.setup_caches(1)
    cur_t, cur_m, pos = tok.unsqueeze(0), msk.unsqueeze(0), torch.arange(tok.shape[0]).unsqueeze(0)
    n_same = n_frames
    for f in range(n_frames):
        tr = C.FrameTrace()
        sf = om.generate_frame(cur_t, cur_m, pos, 1.0, 1, greedy=True, trace=tr)
        if not torch.equal(sf[0], frames[f]):
            top2 = torch.topk(torch.stack(tr.logits, 0)[:, 0].float(), 2, dim=-1)[0]
            _same_until_a_near_tie(frames[f], sf[0], top2[:, 0] - top2[:, 1], noise, f"composed run, frame {f}")
            n_same = f
            break
        cur_t = torch.cat([sf.long(), torch.zeros(1, 1).long()], dim=1).unsqueeze(1)
        cur_m = torch.cat([torch.ones_like(sf).bool(), torch.zeros(1, 1).bool()], dim=1).unsqueeze(1)
        pos = pos[:, -1:] + 1
    ms, mw = M.mimi_full(), M.make_weights(M.mimi_full(), seed=4321)
    # (random weights can pick one of CSM's three codes beyond Mimi's 2,048-entry codebooks; the product clamps them -- mimi_hip.h,
    #  test_codes_beyond_codebook_are_clamped -- where the reference's embedding lookup would raise: the oracle gets them clamped)
    want_own = M.decode(ms, mw, frames.t().unsqueeze(0).long().clamp(max=2047))[0, 0]
    peak = float(want_own.abs().max())
    err_own = float((pcm - want_own).abs().max())
    print(f"composed prompt -> PCM (bench checkpoint): {n_same} of {n_frames} frames identical to the live oracle before a near-tie parts them; "
          f"PCM vs mimi_ref on the same codes: max|d| = {err_own:.3e} = {err_own / peak:.2e} of peak {peak:.3f}")
    assert err_own <= 2e-5 * peak


@pytest.mark.parametrize("B", [1, 8])
@pytest.mark.parametrize("bad", ["inf", "nan"])
def test_non_finite_weights_flow_through_as_non_finite_not_as_a_stalled_launch(csm1b, B, bad):
    """the batched persistent decoder's exchange uses the payload as its own flag (poison 0xFFFFFFFF); a checkpoint
    with an Inf / NaN weight row must not turn into a 50 ms spin + CSM_E_HIP.  Documented outcome (include/csm_hip.h): non-finite
    activations propagate like in the reference (its torch ops do not stall on NaN either): the launch completes at its normal speed, no error
    word is raised, the all-CU paths stay on, every code is inside [0, audio_vocab), and the poisoned row's logits are non-finite."""
    import time
    from sesameai.models import Model, csm_1b_args
    gold, sd = csm1b
    sd = dict(sd)
    w = sd["decoder.layers.1.mlp.w2.weight"].clone()
    w[77] = float("inf") if bad == "inf" else float("nan")                 # one output row of a down projection
    sd["decoder.layers.1.mlp.w2.weight"] = w
    tok, msk = gold["prompt_tokens"], gold["prompt_mask"]
    S = tok.shape[0]
    m = Model(csm_1b_args(), sd, max_frames=16, max_prefill_rows=B * 64)
    m.setup_caches(B)
    want_paths = 1 if B == 1 else 2
    assert m.fast_paths() & want_paths
    m.prefill(tok.unsqueeze(0).repeat(B, 1, 1), msk.unsqueeze(0).repeat(B, 1, 1), torch.arange(S).unsqueeze(0).repeat(B, 1))
    out, logits = m.depth(B, 0.9, 50, want_logits=True, commit=True)
    torch.cuda.synchronize(); t0 = time.perf_counter()
    for _ in range(4):
        m.step(B, 0.9, 50)
    frames, eos = m.read_frames(B)                                          # raises CSM_E_HIP if a launch gave up
    took = time.perf_counter() - t0
    assert m.fast_paths() & want_paths, "the all-CU launch was switched off"
    assert int(frames.min()) >= 0 and int(frames.max()) < 2051
    assert not bool(torch.isfinite(logits[2:].float()).all()), "the non-finite row never reached the logits"
    assert took < 0.04, f"4 frame steps took {took * 1e3:.1f} ms: a launch spun on non-finite payload"


@pytest.mark.parametrize("weights", ["bf16", "fp8"])
def test_tiny_long_context_vs_live_oracle(weights):
    """The tiny shapes with the real 2048-position cache: a 1334-row prompt (flash prompt attention over 1334 keys), then
    frames at p = 1334.. and, from a 1990-row prompt, frames up to the LAST position (2047), HIP vs the live oracle."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from oracle import csm_ref as C
    from sesameai.models import Model, csm_tiny_2k_args, synthetic_state_dict
    shape = C.csm_tiny_2k()
    w = C.make_weights(shape, seed=1234)
    if weights == "fp8":
        w = C.fp8_dequantized(w)
    sd = synthetic_state_dict(csm_tiny_2k_args(), seed=1234)
    m = Model(csm_tiny_2k_args(), sd, max_frames=80, max_prefill_rows=2048, weights_dtype=weights)
    m.setup_caches(1)
    gold = torch.load(os.path.join(GOLD, "tiny_frames.pt"))
    noise = float(gold["bf16_vs_fp32_gap"].max())
    g = torch.Generator().manual_seed(31)
    for S, n_frames in ((1334, 4), (1990, 59)):
        rows_t = torch.zeros(S, 33, dtype=torch.long); rows_m = torch.zeros(S, 33, dtype=torch.bool)
        is_text = torch.rand(S, generator=g) < 0.25
        rows_t[is_text, 32] = torch.randint(0, shape.text_vocab_size, (int(is_text.sum()),), generator=g); rows_m[is_text, 32] = True
        rows_t[~is_text, :32] = torch.randint(0, 2048, (int((~is_text).sum()), 32), generator=g); rows_m[~is_text, :32] = True
        om = C.OracleModel(shape, w); om.setup_caches(1)
        m.reset_caches()
        m.prefill_prompt(rows_t.unsqueeze(0), rows_m.unsqueeze(0))
        cur_t, cur_m, pos = rows_t.unsqueeze(0), rows_m.unsqueeze(0), torch.arange(S).unsqueeze(0)
        worst = 0.0
        for f in range(n_frames):
            tr = C.FrameTrace()
            ref = om.generate_frame(cur_t, cur_m, pos, 1.0, 1, greedy=True, trace=tr)
            want = torch.stack(tr.logits, 0)[:, 0].float()
            check_logits = f < 3 or f >= n_frames - 3
            if check_logits:
                out, logits = m.depth(1, 1.0, 1, forced=ref, want_logits=True, commit=False)
                worst = max(worst, (logits[:, 0].float().cpu() - want).abs().max().item())
                top2 = torch.topk(want, 2, dim=-1)[0]
                for cb in (out[0].cpu() != ref[0]).nonzero().flatten().tolist():
                    assert float(top2[cb, 0] - top2[cb, 1]) <= 2 * noise, (S, f, cb)
            cur_t = torch.cat([ref.long(), torch.zeros(1, 1).long()], dim=1).unsqueeze(1)
            cur_m = torch.cat([torch.ones_like(ref).bool(), torch.zeros(1, 1).bool()], dim=1).unsqueeze(1)
            pos = pos[:, -1:] + 1
            if int(pos[0, 0]) < 2048:
                m.prefill(cur_t, cur_m, pos)                          # one decode row at p = S + f
        print(f"tiny-2k {weights} S={S}: {n_frames} frames up to p={int(pos[0, 0]) - 1}, max|dlogit|={worst:.4f} (noise floor {noise:.4f})")
        assert worst <= 1.25 * noise


# ----------------------------------------------------------------------------------------
# the persistent depth decoder (csrc/dec_persist.cuh): codebooks 2..31 of a batch-1 frame in ONE launch
# ----------------------------------------------------------------------------------------
def test_persistent_decoder_vs_launch_chain_and_golden(csm1b, monkeypatch):
    """Same weights, same prompt, teacher-forced on the golden codes: the persistent launch and the chain of launches
    share every arithmetic step except the summation order of the down projection (split over the 256 workgroups'
    column slices instead of one wave per row), so codebook 0 is bit-identical and codebooks 1..31 agree to a
    few bf16 ulps of the logits -- and both sit inside the oracle's noise floor (checked by the golden tests, which run
    the persistent path by default)."""
    from sesameai.models import Model, csm_1b_args
    gold, sd = csm1b
    tok, msk = gold["prompt_tokens"], gold["prompt_mask"]
    S = tok.shape[0]
    noise = float(gold["bf16_vs_fp32_gap"].max())
    outs = {}
    for name, env in (("persistent", "1"), ("chain", "0")):
        monkeypatch.setenv("CSM_PERSIST", env)
        m = Model(csm_1b_args(), sd, max_frames=64, max_prefill_rows=256)
        m.setup_caches(1)
        m.prefill(tok.unsqueeze(0), msk.unsqueeze(0), torch.arange(S).unsqueeze(0))
        per_frame = []
        for f in range(4):
            out, logits = m.depth(1, 1.0, 1, forced=gold["codes"][f].unsqueeze(0), want_logits=True, commit=False)
            per_frame.append((out.cpu(), logits[:, 0].float().cpu()))
            row = torch.zeros(1, 1, 33, dtype=torch.long); row[0, 0, :32] = gold["codes"][f].long()
            rmask = torch.ones(1, 1, 33, dtype=torch.bool); rmask[0, 0, 32] = False
            m.prefill(row, rmask, torch.tensor([[S + f]]))
        # free-running sampled frames through the captured graph (Philox seeded alike)
        m.reset_caches(); m.seed(4242)
        m.prefill(tok.unsqueeze(0), msk.unsqueeze(0), torch.arange(S).unsqueeze(0))
        m.depth(1, 0.9, 50, commit=True)
        for _ in range(7):
            m.step(1, 0.9, 50)
        frames, eos = m.read_frames(1)
        outs[name] = (per_frame, frames)
        del m
    worst, n_idx = 0.0, 0
    for f in range(4):
        (op, lp), (oc, lc) = outs["persistent"][0][f], outs["chain"][0][f]
        # (round 6: codebook 1 -- the first decoder step, both positions -- runs as ONE all-CU launch too, k_dec_first: same summation-order
        #  differences as the persistent launch; codebook 0 is the backbone's head in both runs)
        assert torch.equal(lp[:1], lc[:1]) and torch.equal(op[0, :1], oc[0, :1]), "codebook 0 does not run in an all-CU decoder launch"
        d = (lp - lc).abs().max().item()
        worst = max(worst, d)
        n_idx += int((op != oc).sum())
        top2 = torch.topk(lc, 2, dim=-1)[0]
        for cb in (op[0] != oc[0]).nonzero().flatten().tolist():
            _excuse(float(top2[cb, 0] - top2[cb, 1]), noise, f"frame {f} codebook {cb}: greedy index differs away from a tie")
    same = (outs["persistent"][1] == outs["chain"][1]).all(dim=2)[:, 0]
    print(f"persistent vs chain: max|dlogit| = {worst:.4f} (oracle noise floor {noise:.4f}); {n_idx} of {4 * 32} greedy indices differ; "
          f"sampled free run: first {int(same.float().cumprod(0).sum())} of {same.numel()} frames identical")
    assert worst <= noise, "the two decoder paths differ by more than the oracle's own bf16-vs-fp32 gap"
    # (sampled free runs part at the first p/q race that a 0.02 logit difference flips -- expected; what must hold is that
    #  the sampler INSIDE the launch is the reference's: next test)


@pytest.mark.parametrize("B", [2, 5, 16, 17, 32])
def test_batched_persistent_decoder_vs_launch_chain(csm1b, monkeypatch, B):
    """The M-row persistent launch (csrc/dec_persist_m.cuh, codebooks 2..31 of B = 2..32 utterances) against the chain of
    launches it replaces, same weights, DIFFERENT prompts per utterance, teacher-forced on random codes: codebooks 0 and 1
    never enter the launch (bit-identical), codebooks 2..31 differ only in fp32 summation order (16 x 16 x 32 matrix ops,
    the MLP's 16-way split) -- logits within the oracle's own bf16-vs-fp32 gap, greedy indices equal away from ties.  Then a
    sampled free run through the captured graph: every frame must be a valid code block and the launch must not give up."""
    import bench
    from oracle import csm_ref as C
    from sesameai.models import Model, csm_1b_args
    gold, sd = csm1b
    noise = float(gold["bf16_vs_fp32_gap"].max())
    tok, msk = bench.synthetic_prompt(_bench_args(), B, C.csm_1b().text_vocab_size, seed0=7000)
    tok, msk = tok[:, :48], msk[:, :48]                          # short prompts: the decoder is what is compared
    S = tok.shape[1]
    g = torch.Generator().manual_seed(B)
    forced = torch.randint(0, 2048, (3, B, 32), generator=g)
    outs = {}
    for name, env in (("persistent", "1"), ("chain", "0")):
        monkeypatch.setenv("CSM_PERSIST_M", env)
        m = Model(csm_1b_args(), sd, max_frames=16, max_prefill_rows=B * S)
        m.setup_caches(B)
        m.prefill(tok, msk, torch.arange(S).unsqueeze(0).repeat(B, 1))
        per_frame = []
        for f in range(3):
            out, logits = m.depth(B, 1.0, 1, forced=forced[f], want_logits=True, commit=False)
            per_frame.append((out.cpu(), logits.float().cpu()))
            row = torch.zeros(B, 1, 33, dtype=torch.long); row[:, 0, :32] = forced[f]
            rmask = torch.ones(B, 1, 33, dtype=torch.bool); rmask[:, 0, 32] = False
            m.prefill(row, rmask, torch.full((B, 1), S + f))
        m.reset_caches(); m.seed(99)
        m.prefill(tok, msk, torch.arange(S).unsqueeze(0).repeat(B, 1))
        m.depth(B, 0.9, 50, commit=True)
        for _ in range(5):
            m.step(B, 0.9, 50)
        frames, eos = m.read_frames(B)                           # raises if a launch gave up
        assert frames.shape == (6, B, 32) and int(frames.min()) >= 0 and int(frames.max()) < 2051
        outs[name] = (per_frame, frames)
        del m
    worst, n_idx = 0.0, 0
    for f in range(3):
        (op, lp), (oc, lc) = outs["persistent"][0][f], outs["chain"][0][f]
        assert torch.equal(lp[:2], lc[:2]) and torch.equal(op[:, :2], oc[:, :2]), "codebooks 0, 1 do not run in the persistent launch"
        worst = max(worst, (lp - lc).abs().max().item())
        top2 = torch.topk(lc, 2, dim=-1)[0]                      # [32][B][2]
        for b, cb in (op != oc).nonzero().tolist():
            n_idx += 1
            _excuse(float(top2[cb, b, 0] - top2[cb, b, 1]), noise, f"frame {f} utterance {b} codebook {cb}: greedy index differs away from a tie")
    same = (outs["persistent"][1] == outs["chain"][1]).all(dim=2).all(dim=1)
    print(f"batched persistent vs chain, B={B}: max|dlogit| = {worst:.4f} (oracle noise floor {noise:.4f}); {n_idx} of {3 * 32 * B} greedy indices differ; "
          f"sampled free run: first {int(same.float().cumprod(0).sum())} of {same.numel()} frames identical")
    assert worst <= 0.5 * noise, "the two decoder paths differ by more than half the oracle's own bf16-vs-fp32 gap (measured 0.28x)"
    assert n_idx <= 0.03 * 3 * 32 * B + 1, "too many greedy picks differ between the two decoder paths"


@pytest.mark.parametrize("B", [3, 8, 32])
def test_split_key_attention_merged_in_kernel_gives_the_merge_launch_bits(csm1b, monkeypatch, B):
    """Batched backbone decode steps split a (row, KV head)'s keys over up to 8 workgroups (csrc/attn.cuh).  The last of them to finish
    merges the partial softmax states itself (default) instead of a second launch (CSM_ATTN_MERGE=0): the same arithmetic in the same
    order, so sampled frames AND logits must be bit-identical, at different positions per row and over several steps (the counters
    must return to zero by themselves)."""
    import bench
    from oracle import csm_ref as C
    from sesameai.models import Model, csm_1b_args
    gold, sd = csm1b
    tok, msk = bench.synthetic_prompt(_bench_args(), B, C.csm_1b().text_vocab_size, seed0=8100)
    tok, msk = tok[:, :150], msk[:, :150]
    S = tok.shape[1]
    outs = {}
    for env in ("1", "0"):
        monkeypatch.setenv("CSM_ATTN_MERGE", env)
        m = Model(csm_1b_args(), sd, max_frames=16, max_prefill_rows=B * S)
        m.setup_caches(B); m.seed(11)
        m.prefill(tok, msk, torch.arange(S).unsqueeze(0).repeat(B, 1))
        m.depth(B, 0.9, 50, commit=True)
        for _ in range(5):
            m.step(B, 0.9, 50)
        frames, _ = m.read_frames(B)
        _, logits = m.depth(B, 1.0, 1, want_logits=True, commit=False)
        outs[env] = (frames.cpu(), logits.float().cpu())
        del m
    assert torch.equal(outs["1"][0], outs["0"][0])
    assert torch.equal(outs["1"][1], outs["0"][1])


def test_two_handles_with_frame_graphs_of_different_shapes_do_not_disturb_each_other(csm1b, monkeypatch):
    """Round 4 regression (found by tools/soak_attn_merge.py): with the batched persistent decoder's exchange buffers poisoned by a MEMSET node
    of the captured frame step, a handle replaying its graph beside a second handle whose graph has another shape (here: split-key attention
    merged by a second launch vs in the kernel) produced garbage from codebook 2 on -- its launch ran on exchange buffers that were not poisoned
    yet; eager launches were fine.  The poison is written by a kernel node now.  Two B = 32 handles, run alternately three times with the same
    seed: every run of a handle equals its first, and the two handles (same arithmetic, same order) equal each other."""
    import bench
    from oracle import csm_ref as C
    from sesameai.models import Model, csm_1b_args
    gold, sd = csm1b
    B = 32
    tok, msk = bench.synthetic_prompt(_bench_args(), B, C.csm_1b().text_vocab_size, seed0=9100 + B)
    tok, msk = tok[:, :100], msk[:, :100]
    S = tok.shape[1]
    handles = []
    for env in ("0", "1"):
        monkeypatch.setenv("CSM_ATTN_MERGE", env)
        m = Model(csm_1b_args(), sd, max_frames=16, max_prefill_rows=B * S)
        m.setup_caches(B)
        assert m.fast_paths() & 2
        handles.append(m)

    def run(m):
        m.reset_caches(); m.seed(778)
        m.prefill(tok, msk, torch.arange(S).unsqueeze(0).repeat(B, 1))
        m.depth(B, 0.9, 50, commit=True)
        for _ in range(6):
            m.step(B, 0.9, 50)
        return m.read_frames(B)[0]

    out = [[run(m) for m in handles] for _ in range(3)]
    for rep in range(3):
        assert torch.equal(out[rep][0], out[0][0]) and torch.equal(out[rep][1], out[0][1]), f"run {rep} of a handle differs from its first run"
        assert torch.equal(out[rep][0], out[rep][1]), "the two handles differ"


_FAULT_SCRIPT = r"""
import os, sys, time
os.environ["CSM_HIP_TIMELINE"] = "1"          # the library build that carries the fault-injection hook
os.environ["CSM_PERSIST_FAULT"] = "1"         # the first persistent launch withholds one hand-off granule
root = sys.argv[1]
sys.path.insert(0, root); sys.path.insert(0, os.path.join(root, "sesameai-tts_amd"))
import torch
from sesameai.models import Model, csm_1b_args, synthetic_state_dict
margs = csm_1b_args()
m = Model(margs, synthetic_state_dict(margs, seed=1234), max_frames=16, max_prefill_rows=256)
m.setup_caches(1); m.seed(3)
g = torch.Generator().manual_seed(0)
S = 20
tok = torch.zeros(1, S, 33, dtype=torch.long); tok[0, :, :32] = torch.randint(0, 2048, (S, 32), generator=g)
msk = torch.ones(1, S, 33, dtype=torch.bool); msk[0, :, 32] = False
def run():
    m.reset_caches(); m.seed(3)
    m.prefill(tok, msk, torch.arange(S).unsqueeze(0))
    m.depth(1, 0.9, 50, commit=True)
    for _ in range(3): m.step(1, 0.9, 50)
    return m.read_frames(1)[0].clone()
t0 = time.perf_counter()
# the reference-style loop never calls read_frames: the frame it copies out (generate_frame -> csm_copy_frame) must say so itself
m.reset_caches(); m.seed(3)
m.prefill(tok, msk, torch.arange(S).unsqueeze(0))
first = m.depth(1, 0.9, 50, commit=True)
row = torch.zeros(1, 1, 33, dtype=torch.long); row[0, 0, :32] = first[0].clamp(min=0).long().cpu()
rmask = torch.ones(1, 1, 33, dtype=torch.bool); rmask[0, 0, 32] = False
nxt = m.generate_frame(row, rmask, torch.tensor([[S]]), 0.9, 50)
print("FRAME_MARKED_INVALID" if int(first.min()) == -1 or int(nxt.min()) == -1 else "FRAME_NOT_MARKED", first[0, :4].tolist(), nxt[0, :4].tolist())
try:
    m.read_frames(1); torch.cuda.synchronize()
    print("NO_ERROR")
except RuntimeError as e:
    print("ERROR_OK" if "gave up" in str(e) else "OTHER_ERROR " + str(e), f"{time.perf_counter() - t0:.2f}s")
a = run(); b = run()
print("RECOVERED" if torch.equal(a, b) and int(a.min()) >= 0 and int(a.abs().sum()) > 0 else "NOT_RECOVERED")
"""


def test_persistent_launch_gives_up_instead_of_hanging_and_the_handle_recovers(tmp_path):
    """Every spin of the persistent launch is bounded: with one hand-off granule withheld (fault injection of the
    timeline build, CSM_PERSIST_FAULT) the launch must END within its 50 ms budget, read_frames must report it
    (CSM_E_HIP, "gave up"), every host-visible copy of the invalid frame must carry -1 (the reference-style loop reads frames
    through generate_frame and never calls read_frames), and after reset_caches the same handle must generate again."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    lib = os.path.join(root, "sesameai-tts_amd", "lib", "libcsm_hip_timeline.so")
    if not os.path.exists(lib):
        pytest.skip("libcsm_hip_timeline.so not built (make -C sesameai-tts_amd/csrc timeline)")
    script = tmp_path / "fault.py"
    script.write_text(_FAULT_SCRIPT)
    # default: after a give-up the handle falls back to the launch chain; CSM_KEEP_FAST_PATHS=1: the persistent launch itself must
    # work again after reset_caches (the tag epoch moves past whatever the aborted launch left in the granule buffers)
    for keep in ("0", "1"):
        env = dict(os.environ)
        env.pop("CSM_KEEP_FAST_PATHS", None)
        if keep == "1":
            env["CSM_KEEP_FAST_PATHS"] = "1"
        r = subprocess.run([sys.executable, str(script), root], capture_output=True, text=True, timeout=240, env=env)
        out = r.stdout
        assert "FRAME_MARKED_INVALID" in out, f"keep={keep}: generate_frame returned codes of a launch that gave up without marking them (-1):\n{out}\n{r.stderr[-2000:]}"
        assert "ERROR_OK" in out, f"keep={keep}: the faulted launch was not reported:\n{out}\n{r.stderr[-2000:]}"
        assert "RECOVERED" in out and "NOT_RECOVERED" not in out, f"keep={keep}: the handle did not recover:\n{out}\n{r.stderr[-2000:]}"


def test_first_decoder_step_as_one_launch_vs_its_launch_chain(csm1b, monkeypatch):
    """Codebook 1 -- the decoder's first step, positions 0 and 1 -- as ONE all-CU launch (csrc/dec_first.cuh, round 6) against the 16 launches of
    the M = 2 chain + the head GEMV it replaces (CSM_DEC_FIRST=0), the persistent launch for codebooks 2..31 on both sides.  Same rounding points,
    different fp32 summation orders (gate/up on the matrix cores, the down projection split over 256 column slices): codebook 0 bit-identical,
    codebook 1's logits and -- through the K / V rows of positions 0, 1 that the launch files in the decoder caches -- every later codebook's
    within the oracle's own bf16-vs-fp32 gap; greedy picks may differ only at near-ties; and the launch is deterministic."""
    from sesameai.models import Model, csm_1b_args
    gold, sd = csm1b
    tok, msk = gold["prompt_tokens"], gold["prompt_mask"]
    S = tok.shape[0]
    noise = float(gold["bf16_vs_fp32_gap"].max())
    outs = {}
    for name, env in (("one launch", "1"), ("chain", "0")):
        monkeypatch.setenv("CSM_DEC_FIRST", env)
        m = Model(csm_1b_args(), sd, max_frames=16, max_prefill_rows=256)
        m.setup_caches(1)
        assert bool(m.fast_paths() & 32) == (env == "1") and m.fast_paths() & 1
        m.prefill(tok.unsqueeze(0), msk.unsqueeze(0), torch.arange(S).unsqueeze(0))
        res = []
        for f in range(3):
            out, logits = m.depth(1, 1.0, 1, forced=gold["codes"][f].unsqueeze(0), want_logits=True, commit=False)
            out2, logits2 = m.depth(1, 1.0, 1, forced=gold["codes"][f].unsqueeze(0), want_logits=True, commit=False)
            assert torch.equal(logits, logits2) and torch.equal(out, out2), "not deterministic"
            res.append((out.cpu(), logits[:, 0].float().cpu()))
            row = torch.zeros(1, 1, 33, dtype=torch.long); row[0, 0, :32] = gold["codes"][f].long()
            rmask = torch.ones(1, 1, 33, dtype=torch.bool); rmask[0, 0, 32] = False
            m.prefill(row, rmask, torch.tensor([[S + f]]))
        outs[name] = res
        del m
    worst1 = worst = 0.0
    for (oa, la), (ob, lb) in zip(outs["one launch"], outs["chain"]):
        assert torch.equal(la[0], lb[0]), "codebook 0 is the backbone's head on both sides"
        worst1 = max(worst1, (la[1] - lb[1]).abs().max().item())
        worst = max(worst, (la - lb).abs().max().item())
        top2 = torch.topk(lb, 2, dim=-1)[0]
        for cb in (oa[0] != ob[0]).nonzero().flatten().tolist():
            _excuse(float(top2[cb, 0] - top2[cb, 1]), noise, f"codebook {cb}: greedy index differs away from a tie")
    print(f"first decoder step, one launch vs chain: max|dlogit| codebook 1 = {worst1:.4f}, any codebook = {worst:.4f} (oracle noise floor {noise:.4f})")
    assert worst1 > 0.0, "both runs took the same path"
    assert worst <= noise


def test_backbone_attention_block_vs_launch_chain(csm1b, monkeypatch):
    """Batch-1 decode steps run q|k|v -> attention -> o-projection of every backbone layer as ONE launch
    (csrc/bb_block.cuh) instead of three.  Same rounding points, different fp32 summation orders (per-wave RMSNorm sums,
    attention over 8 waves x 8 key slots instead of split-K blocks): teacher-forced on the golden codes through the
    graph step, the logits of both paths must agree within the oracle's own bf16-vs-fp32 gap and greedy picks may differ
    only at near-ties.  Also at a long context (keys beyond the 768 prefetched at kernel entry)."""
    from sesameai.models import Model, csm_1b_args
    gold, sd = csm1b
    tok, msk = gold["prompt_tokens"], gold["prompt_mask"]
    S = tok.shape[0]
    noise = float(gold["bf16_vs_fp32_gap"].max())
    g = torch.Generator().manual_seed(5)
    long_S = 900
    ltok = torch.zeros(long_S, 33, dtype=torch.long); ltok[:, :32] = torch.randint(0, 2048, (long_S, 32), generator=g)
    lmsk = torch.ones(long_S, 33, dtype=torch.bool); lmsk[:, 32] = False
    outs = {}
    for name, env in (("block", "1"), ("chain", "0")):
        monkeypatch.setenv("CSM_BB_BLOCK", env)
        m = Model(csm_1b_args(), sd, max_frames=16, max_prefill_rows=1024)
        m.setup_caches(1)
        res = []
        for (t_, m_, S_) in ((tok, msk, S), (ltok, lmsk, long_S)):
            m.reset_caches()
            m.prefill(t_.unsqueeze(0), m_.unsqueeze(0), torch.arange(S_).unsqueeze(0))
            m.depth(1, 1.0, 1, forced=gold["codes"][0].unsqueeze(0), commit=True)
            for f in range(1, 4):
                row = torch.zeros(1, 1, 33, dtype=torch.long); row[0, 0, :32] = gold["codes"][f - 1].long()
                rmask = torch.ones(1, 1, 33, dtype=torch.bool); rmask[0, 0, 32] = False
                m.prefill(row, rmask, torch.tensor([[S_ + f - 1]]))          # one-row decode step of the backbone (narrow path)
                out, logits = m.depth(1, 1.0, 1, forced=gold["codes"][f].unsqueeze(0), want_logits=True, commit=False)
                res.append((out.cpu(), logits[:, 0].float().cpu()))
        outs[name] = res
        del m
    worst = 0.0
    for (ob, lb), (oc, lc) in zip(outs["block"], outs["chain"]):
        worst = max(worst, (lb - lc).abs().max().item())
        top2 = torch.topk(lc, 2, dim=-1)[0]
        for cb in (ob[0] != oc[0]).nonzero().flatten().tolist():
            _excuse(float(top2[cb, 0] - top2[cb, 1]), noise, f"codebook {cb}: greedy index differs away from a tie")
    print(f"backbone block vs chain: max|dlogit| = {worst:.4f} (oracle noise floor {noise:.4f})")
    assert worst > 0.0, "both runs took the same path"
    assert worst <= noise


def test_persistent_decoder_samples_like_the_oracle_on_its_own_logits(csm1b):
    """The sampler runs inside the persistent launch (on every CU alike).  Given Exp(1) noise, its picks for codebooks
    2..31 must be the oracle's sample_topk of the very logits the launch produced (misses only at 1-ulp ties of p/q),
    and the codes fed to the next step are the picks: a second call fed the same noise reproduces them exactly."""
    from oracle.csm_ref import sample_topk
    from sesameai.models import Model, csm_1b_args
    from gpu_util import bf16_ulp_diff
    import torch.nn.functional as F
    gold, sd = csm1b
    tok, msk = gold["prompt_tokens"], gold["prompt_mask"]
    S = tok.shape[0]
    V = 2051
    m = Model(csm_1b_args(), sd, max_frames=16, max_prefill_rows=256)
    m.setup_caches(1)
    m.prefill(tok.unsqueeze(0), msk.unsqueeze(0), torch.arange(S).unsqueeze(0))
    g = torch.Generator().manual_seed(77)
    total = agree = 0
    for (T, k) in ((0.9, 50), (0.7, 30), (1.0, 2051), (1.3, 5)):
        noise = torch.empty(32, 1, V).exponential_(1, generator=g).to(torch.bfloat16).clamp_min(1e-30)
        out, logits = m.depth(1, T, k, noise=noise, want_logits=True, commit=False)
        out2 = m.depth(1, T, k, noise=noise, commit=False)
        assert torch.equal(out, out2), "the persistent launch is not deterministic"
        lg = logits[:, 0].cpu()                                     # [32][V] bf16: the logits the launch sampled from
        want = sample_topk(lg, k, T, q=noise[:, 0])[:, 0]
        got = out[0].cpu()
        bad = (got != want).nonzero().flatten()
        for cb in bad.tolist():
            l = lg[cb:cb + 1] / T
            kth = torch.topk(l, k)[0][..., -1, None]
            probs = F.softmax(F.log_softmax(l.masked_fill(l < kth, -float("inf")), dim=-1), dim=-1)
            r = (probs / noise[cb])[0]
            assert int(bf16_ulp_diff(r[got[cb].long()], r[want[cb].long()]).max()) <= 1, f"T={T} k={k} codebook {cb}: not a 1-ulp tie"
        total += 32; agree += 32 - int(bad.numel())
    print(f"sampler inside the persistent launch: {agree}/{total} picks identical to the oracle's on the launch's logits")
    assert agree / total >= 0.95


def test_model_from_pretrained_reads_reference_and_transformers_checkpoints(tmp_path, csm1b):
    """Model.from_pretrained (reference: PyTorchModelHubMixin.from_pretrained("sesame/csm-1b"), sesameai/generator.py:338):
    a local model.safetensors in the reference's (torchtune) tensor names gives the same frames as the state dict
    itself.  (The transformers-format branch is the name / RoPE-row conversion tested in test_host_logic.)"""
    from safetensors.torch import save_file
    from sesameai.models import Model, csm_1b_args
    gold, sd = csm1b
    d = tmp_path / "csm-1b"
    d.mkdir()
    save_file({k: v.contiguous() for k, v in sd.items()}, str(d / "model.safetensors"))
    tok, msk = gold["prompt_tokens"], gold["prompt_mask"]
    S = tok.shape[0]
    outs = []
    for m in (Model.from_pretrained(str(d), device="cuda", max_frames=8, max_prefill_rows=64),
              Model(csm_1b_args(), sd, max_frames=8, max_prefill_rows=64)):
        m.setup_caches(1)
        m.prefill(tok.unsqueeze(0), msk.unsqueeze(0), torch.arange(S).unsqueeze(0))
        out, logits = m.depth(1, 1.0, 1, want_logits=True, commit=False)
        outs.append((out.cpu(), logits.cpu()))
        del m
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
