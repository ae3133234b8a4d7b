"""Free-running greedy codes that are read out of the DEPTH DECODER's KV cache, bit-identical to the oracle's, with no excused row.

`decisive` and `decisive_copy` keep c_i = perm_i^-1[c_(i-1)]: one row's residual stream, no cached key.  In the decoder-copy checkpoint
(oracle.csm_ref.decisive_dcopy_variant, flavour "decisive_dcopy:<layer>:<lag>") step p > lag emits perm_p^-1[c_(p-1-lag)], read through the
RoPE'd cached K and the cached V of position p - lag in ONE decoder layer.  oracle/make_golden.py asserts on the oracle that a stale row, a K
rotated one position off, K / V appended one slot off, zeroed first-call rows or hidden keys in that layer change these trajectories
(tests/test_dcopy_oracle.py re-asserts it), and margin >= 4 x the oracle's bf16-vs-fp32 gap on every decision.  The variants at CSM-1B shapes:
    :0:1  the table-fed layer; every step reads the key the step before wrote (p = 2 reads position 1, written by k_dec_first);
    :3:2  the last layer; p = 3 reads position 1 -- k_dec_first's, handed to k_dec_persist through global memory; also with the fp8 weight stream;
    :1:7  a middle layer, a key seven back among more competitors.
The construction lives in the oracle alone: the checkpoint is built with oracle.csm_ref and handed to Model(...) as a state dict, after every
tensor's checksum is compared with the golden's.  8 frames at B = 1, 4 at B > 1: every frame is 31 decoder steps on a cache that starts empty."""
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
V01, V32, V17 = "decisive_dcopy:0:1", "decisive_dcopy:3:2", "decisive_dcopy:1:7"


@pytest.fixture(scope="module")
def dcopy():
    """(golden, get(flavour) -> state dict): the draws and the shared base are built once per module, one variant is kept at a time."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from oracle import csm_ref as C
    from oracle.make_golden import weight_checksums
    gold = torch.load(os.path.join(GOLD, "csm1b_decisive_dcopy.pt"))
    shape, seed = C.csm_1b(), int(gold["weight_seed"])
    built = {}

    def get(flavour):
        if flavour not in built:
            if "w" not in built:
                built["w"] = C.make_weights(shape, seed=seed)
                built["base"] = C.decisive_dcopy_base(shape, built["w"], seed)
            for k in [k for k in built if k not in ("w", "base")]:
                del built[k]
            layer, lag = C.dcopy_flavour_params(shape, flavour)
            sd = C.decisive_dcopy_variant(shape, built["base"], built["w"], seed, layer, lag)
            names, sums = gold["weight_checksums"][flavour]
            got = weight_checksums(sd)
            bad = [k for k, a, b in zip(names, got[1].tolist(), sums.tolist()) if a != b]
            assert got[0] == names and not bad, f"{flavour}: this host builds another checkpoint than the one the oracle's codes were generated with: {bad[:4]}"
            built[flavour] = sd
        return built[flavour]
    yield gold, get
    built.clear()


def _model(sd, batch=1, rows=2048, dtype="bf16"):
    from sesameai.models import Model, csm_1b_args
    m = Model(csm_1b_args(), sd, max_frames=16, max_prefill_rows=rows, weights_dtype=dtype)
    m.setup_caches(batch)
    return m


def _report(what, flavour, g):
    line = f"\n[dcopy] {what} ({flavour}): {g['codes'].shape[0]} free-running frames bit-identical to the oracle; smallest oracle margin " \
           f"{float(g['min_margin'].min()):.2f} = {float(g['min_margin'].min() / g['max_gap'].max()):.0f} x its bf16-vs-fp32 gap"
    if "faults_changed" in g:
        line += f"; oracle KV faults {g['kinds']} moved {g['faults_changed'].tolist()} of its frames in the copy layer, {g['other_layer_changed'].tolist()} in another"
    print(line)


def _first_difference(got, want):
    return f"first difference at {(got != want).nonzero()[0].tolist()}" if got.shape == want.shape else f"{tuple(got.shape)} frames"


def _reference_style_loop(m, tok, msk, n):
    m.reset_caches()
    dev = m.device
    curr_tokens, curr_mask = tok.unsqueeze(0).to(dev), msk.unsqueeze(0).to(dev)
    curr_pos = torch.arange(0, tok.size(0)).unsqueeze(0).long().to(dev)
    samples = []
    for _ in range(n):
        sample = m.generate_frame(curr_tokens, curr_mask, curr_pos, 1.0, 1)
        samples.append(sample)
        curr_tokens = torch.cat([sample, torch.zeros(1, 1).long().to(dev)], dim=1).unsqueeze(1)
        curr_mask = torch.cat([torch.ones_like(sample).bool(), torch.zeros(1, 1).bool().to(dev)], dim=1).unsqueeze(1)
        curr_pos = curr_pos[:, -1:] + 1
    return torch.cat(samples).cpu()


def _b1(dcopy, monkeypatch, flavour, leg, dtype="bf16"):
    from test_decisive_gpu import _generator, _prompts
    gold, get = dcopy
    g = gold["runs"][flavour][f"{dtype}_s190"]
    want = g["codes"][:, 0].to(torch.int32)
    tok, msk = _prompts(128_256)["s190"]
    assert want.shape == (8, 32) and tok.shape[0] == int(gold["prompt_rows"]) and bool((g["faults_changed"] > 0).all())
    if leg == "dec_first_off":
        monkeypatch.setenv("CSM_DEC_FIRST", "0")
    if leg == "chain":
        monkeypatch.setenv("CSM_PERSIST", "0")
    m = _model(get(flavour), dtype=dtype)
    paths = m.fast_paths()
    assert paths & (8 if dtype == "bf16" else 16), "the one-launch backbone layer did not run"
    assert bool(paths & 1) == (leg != "chain") and bool(paths & 32) == (leg not in ("chain", "dec_first_off")), f"fast paths {paths} are not the ones {leg} means"
    if leg == "reference_loop":
        got = _reference_style_loop(m, tok, msk, want.shape[0])
    else:
        got = _generator(m).generate_codes(tok, msk, want.shape[0], 1.0, 1)[:, 0].cpu()
    assert torch.equal(got, want), f"{flavour} {dtype} {leg}: (frame, codebook) " + _first_difference(got, want)
    _report(f"B = 1 {dtype} {leg}", flavour, g)


def _batched(dcopy, flavour, B):
    import bench
    from oracle import csm_ref as C
    from oracle.make_golden import dcopy_prompts
    from test_decisive_gpu import _bench_args
    gold, get = dcopy
    g = gold["runs"][flavour]["bf16_b32"]
    all_codes = g["codes"].to(torch.int32)                                        # [4][32][32]
    assert all_codes.shape == (4, 32, 32)
    first = all_codes[0]
    assert all(not torch.equal(first[i], first[j]) for i in range(32) for j in range(i)), "two utterances of the golden batch share a first frame"
    # (the batched oracle computes every utterance on its own rows: the first B utterances of its batch of 32 are the oracle's batch of B)
    want = all_codes[:, :B]
    batch = dcopy_prompts(C.csm_1b(), full=True)[1][:B]              # config 3's prompts, every utterance with a last text token of its own
    tok, msk = torch.stack([p[0] for p in batch]), torch.stack([p[1] for p in batch])
    ref = bench.synthetic_prompt(_bench_args(), B, 128_256, seed0=2025)
    assert torch.equal(tok[:, :-1], ref[0][:, :-1]) and torch.equal(msk, ref[1]) and torch.equal(tok.sum(dim=(1, 2)), g["prompt_checksum"][:B])
    S = tok.shape[1]
    m = _model(get(flavour), B, rows=B * S)
    assert m.fast_paths() & 2, "the batched persistent decoder does not run"
    m.prefill(tok, msk, torch.arange(S).unsqueeze(0).repeat(B, 1))
    m.depth(B, 1.0, 1, commit=True)
    for _ in range(want.shape[0] - 1):
        m.step(B, 1.0, 1)
    fr, eos = m.read_frames(B)
    assert bool((eos < 0).all())
    assert torch.equal(fr, want), f"{flavour} B = {B}: {int((fr != want).any(dim=2).sum())} of {want.shape[0] * B} frames differ; (frame, utterance, codebook) " + _first_difference(fr, want)
    _report(f"B = {B}", flavour, g)


# ---- the table-fed layer, lag 1 (the tests are grouped by variant: one checkpoint is built at a time) ------------------------------
@pytest.mark.parametrize("leg", ["graph", "reference_loop", "dec_first_off", "chain"])
def test_b1_table_fed_layer(dcopy, monkeypatch, leg):
    """The 190-row prompt at B = 1.  `graph`: generate_codes (prefill -> frame 0 -> the hipGraph frame loop) on k_dec_first + k_dec_persist;
    `reference_loop`: one generate_frame per frame; `dec_first_off`: CSM_DEC_FIRST=0, the persistent launch without the global-memory
    hand-over of positions 0 and 1; `chain`: CSM_PERSIST=0, the launch chain (k_attn, the fused attention + o-proj) at CSM-1B shapes."""
    _b1(dcopy, monkeypatch, V01, leg)


@pytest.mark.parametrize("B", [4, 17, 32])
def test_batched_persistent_decoder_table_fed_layer(dcopy, B):
    """k_dec_persist_m's cache per (row, head) owner: one 16-row half, two, and config 3's batch; every utterance a prompt of its own."""
    _batched(dcopy, V01, B)


@pytest.mark.parametrize("beside", [True, False])
def test_refilled_batch_of_8(dcopy, beside):
    """Twelve utterances through 8 slots that are kept full, both refill paths: the decoder cache of a slot that was just refilled."""
    from oracle import csm_ref as C
    from oracle.make_golden import dcopy_many_prompts
    from test_decisive_gpu import _generator
    gold, get = dcopy
    many = gold["runs"][V01]["bf16_many"]
    want = [r["codes"].to(torch.int32) for r in many]
    spec = dcopy_many_prompts(C.csm_1b())
    prompts, limits = [p for p, _ in spec], [lim for _, lim in spec]
    assert [w.shape[0] for w in want] == limits
    m = _model(get(V01), 8)
    gen = _generator(m, batch=8)
    gen.refill_beside_the_loop = beside
    got = gen.generate_codes_continuous(prompts, limits, 1.0, 1)
    for i, (a, b) in enumerate(zip(got, want)):
        assert torch.equal(a.cpu(), b), f"utterance {i} (S={prompts[i][0].shape[0]}, {limits[i]} frames, refill beside the loop = {beside}): " + _first_difference(a.cpu(), b)
    assert m.fast_paths() & 2, "the batched persistent decoder did not run"
    worst = min(float(r["min_margin"].min() / r["max_gap"].max()) for r in many)
    print(f"\n[dcopy] refilled batch of 8 (beside the loop = {beside}): 12 utterances bit-identical; smallest oracle margin {worst:.0f} x the gap")


def test_plain_c_host(dcopy, tmp_path):
    """examples/c_host/csm_c_host.c (no Python in the process): its blob writer takes the handle as it is, whatever state dict built it."""
    from test_c_host_gpu import run_greedy_host
    from test_decisive_gpu import _prompts
    gold, get = dcopy
    want = gold["runs"][V01]["bf16_s190"]["codes"][:, 0].to(torch.int32)
    tok, msk = _prompts(128_256)["s190"]
    got, after = run_greedy_host(_model(get(V01)), tok, msk, want.shape[0], str(tmp_path / "csm1b_decisive_dcopy.blob"))
    assert after == "eos_at -1"
    assert torch.equal(got, want), "(frame, codebook) " + _first_difference(got, want)


# ---- the last layer, lag 2: p = 3 reads position 1, k_dec_first's, which k_dec_persist gets through global memory -----------------------
@pytest.mark.parametrize("dtype,leg", [("bf16", "graph"), ("fp8", "graph"), ("bf16", "dec_first_off"), ("bf16", "chain")])
def test_b1_last_layer(dcopy, monkeypatch, dtype, leg):
    _b1(dcopy, monkeypatch, V32, leg, dtype)


# ---- a middle layer, lag 7 ---------------------------------------------------------------------------------------------------------------
def test_b1_middle_layer(dcopy, monkeypatch):
    _b1(dcopy, monkeypatch, V17, "graph")


@pytest.mark.parametrize("B", [4, 17, 32])
def test_batched_persistent_decoder_middle_layer(dcopy, B):
    _batched(dcopy, V17, B)


# ---- tiny shapes: the launch chain (k_attn, the fused attention + o-proj) ------------------------------------------------------------
@pytest.mark.parametrize("flavour", ["decisive_dcopy:0:1", "decisive_dcopy:1:3"])
@pytest.mark.parametrize("batched", [False, True])
def test_tiny_shapes(flavour, batched):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from oracle import csm_ref as C
    from oracle.make_golden import dcopy_prompts, weight_checksums
    from sesameai.models import Model, csm_tiny_args
    from test_decisive_gpu import _generator
    gold = torch.load(os.path.join(GOLD, "tiny_decisive_dcopy.pt"))
    shape = C.csm_tiny()
    (tok, msk), batch = dcopy_prompts(shape, full=False)
    sd = C.make_weights(shape, seed=int(gold["weight_seed"]), flavour=flavour)
    names, sums = gold["weight_checksums"][flavour]
    got = weight_checksums(sd)
    assert got[0] == names and torch.equal(got[1], sums), f"{flavour}: this host builds another checkpoint than the golden's"
    B = len(batch) if batched else 1
    m = Model(csm_tiny_args(), sd, max_frames=16, max_prefill_rows=1024)
    m.setup_caches(B)
    assert not m.fast_paths() & (1 | 2 | 32), "the tiny shapes are meant to run the decoder's launch chain"
    gen = _generator(m, batch=B)
    g = gold["runs"][flavour]["bf16_b32" if batched else "bf16_s190"]
    want = g["codes"].to(torch.int32)
    if batched:
        got = gen.generate_codes(torch.stack([p[0] for p in batch]), torch.stack([p[1] for p in batch]), want.shape[0], 1.0, 1).cpu()
    else:
        got = gen.generate_codes(tok, msk, want.shape[0], 1.0, 1).cpu()
    assert torch.equal(got, want), f"tiny {flavour} B = {B}: (frame, utterance, codebook) " + _first_difference(got, want)
    _report(f"tiny B = {B}", flavour, g)
