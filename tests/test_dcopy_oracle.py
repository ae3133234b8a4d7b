"""CPU side of the decoder-copy checkpoint (oracle.csm_ref.decisive_dcopy_base / decisive_dcopy_variant): free-running greedy codes that are
read out of ONE depth-decoder layer's KV cache.  The oracle's trajectory is the one the construction implies and the one committed under
tests/golden/; KV faults injected into that decoder layer of the ORACLE change it, the same faults in another decoder layer or in the
backbone do not, and the two older decisive flavours see none of the decoder faults (the gap this flavour closes); every stored decision
has margin >= 4 x the oracle's own bf16-vs-fp32 gap.  tests/test_dcopy_gpu.py holds the HIP path to those codes bit for bit."""
import os

import torch

GOLD = os.path.join(os.path.dirname(__file__), "golden")
FILES = ("tiny_decisive_dcopy.pt", "csm1b_decisive_dcopy.pt")


def _run(shape, model, tok, msk, n):
    from oracle import csm_ref as C
    return torch.cat(C.generate_codes(model, tok, msk, n * 80, 1.0, 1, greedy=True, max_seq_len=shape.backbone.max_seq_len))


def test_dcopy_free_run_follows_the_construction_and_the_golden():
    from oracle import csm_ref as C
    from oracle.make_golden import dcopy_prompts, weight_checksums
    shape = C.csm_tiny()
    gold = torch.load(os.path.join(GOLD, FILES[0]))
    seed = int(gold["weight_seed"])
    (tok, msk), _ = dcopy_prompts(shape, full=False)
    w = C.make_weights(shape, seed=seed)
    base = C.decisive_dcopy_base(shape, w, seed)
    for flavour in gold["variants"]:
        layer, lag = C.dcopy_flavour_params(shape, flavour)
        wts = C.decisive_dcopy_variant(shape, base, w, seed, layer, lag)
        whole = C.make_weights(shape, seed=seed, flavour=flavour)
        assert set(whole) == set(wts) and all(torch.equal(whole[k], wts[k]) for k in wts), flavour
        names, sums = gold["weight_checksums"][flavour]
        assert names == sorted(wts) and torch.equal(weight_checksums(wts)[1], sums), f"{flavour}: this host builds another checkpoint than the golden's"
        # variants differ from their base in one decoder layer's q / k / output_proj and in audio_head alone
        differ = sorted(k for k in wts if not torch.equal(wts[k], base[k]))
        assert differ == sorted([f"decoder.layers.{layer}.attn.{t}_proj.weight" for t in ("q", "k", "output")] + ["audio_head"]), differ
        m = C.OracleModel(shape, wts)
        m.setup_caches(1)
        n = 8
        frames = _run(shape, m, tok, msk, n)
        assert torch.equal(frames, C.decisive_dcopy_expected_codes(shape, seed, int(tok[-1, 32]), n, lag)), flavour
        assert torch.equal(frames, gold["runs"][flavour]["bf16_s190"]["codes"][:n, 0].to(torch.int32)), flavour


def test_decoder_kv_faults_move_the_dcopy_trajectory_and_no_other():
    """The tiny fault matrix, live.  In the copy layer of the DECODER every fault kind -- steps that do not append their K / V, a K rotated
    one position off either way, K / V appended one slot off, the first call's two rows zeroed, the copied-from keys hidden -- changes the
    free-running codes; in the other decoder layer and in a backbone layer none does; and none of the decoder faults moves `decisive` or
    `decisive_copy` (their decoder chain follows one row's residual stream and never reads a cached key)."""
    from oracle import csm_ref as C
    from oracle.make_golden import dcopy_backbone_faults, dcopy_decoder_faults, dcopy_prompts, fault_name, faulted_frames
    shape = C.csm_tiny()
    (tok, msk), _ = dcopy_prompts(shape, full=False)
    n = 4
    for flavour in ("decisive_dcopy:0:1", "decisive_dcopy:1:3", "decisive", "decisive_copy"):
        m = C.OracleModel(shape, C.make_weights(shape, seed=1234, flavour=flavour))
        m.setup_caches(1)
        want = _run(shape, m, tok, msk, n)
        is_dcopy = flavour.startswith("decisive_dcopy")
        layer, lag = C.dcopy_flavour_params(shape, flavour) if is_dcopy else (None, 2)
        faults = dcopy_decoder_faults(shape, lag)
        for L in range(shape.decoder.num_layers):
            changed = faulted_frames(m, shape, tok, msk, want, "decoder", L, faults)
            print(f"\n[dcopy-oracle] {flavour}: faults {[fault_name(f) for f in faults]} in decoder layer {L} change {changed.tolist()} of {n} frames")
            assert bool((changed > 0).all()) if L == layer else not bool(changed.any()), (flavour, L, changed.tolist())
        if is_dcopy:
            changed = faulted_frames(m, shape, tok, msk, want, "backbone", 1, dcopy_backbone_faults(tok.shape[0], n))
            assert not bool(changed.any()), (flavour, "backbone", changed.tolist())
        assert C.KV_FAULT is None


def test_every_stored_dcopy_trajectory_was_decided_with_room_to_spare_and_saw_the_faults():
    for fname in FILES:
        path = os.path.join(GOLD, fname)
        assert os.path.getsize(path) < 1 << 20
        gold = torch.load(path)
        assert set(gold["runs"]) == set(gold["variants"]) == set(gold["weight_checksums"])
        for flavour, runs in gold["runs"].items():
            for key, g in runs.items():
                for r in (g if isinstance(g, list) else [g]):
                    codes = r["codes"] if r["codes"].dim() == 3 else r["codes"].unsqueeze(1)
                    assert float(r["min_margin"].min()) >= 4.0 * float(r["max_gap"].max()), (fname, flavour, key)
                    assert int(codes.max()) < 2048 and int(codes.min()) >= 0 and not bool((codes == 0).all(dim=2).any())
                    if "margin" in r:           # per (frame, codebook, utterance)
                        assert r["margin"].shape == r["gap"].shape == (codes.shape[0], 32, codes.shape[1])
                        assert float(r["margin"].min()) >= 4.0 * float(r["gap"].max())
                if key.endswith("_s190"):
                    assert g["codes"].shape[:2] == (8, 1)
                    assert bool((g["faults_changed"] > 0).all()) and not bool(g["other_layer_changed"].any()), (fname, flavour, key)
                    assert "backbone_changed" not in g or not bool(g["backbone_changed"].any())
                    print(f"\n[dcopy-oracle] {fname} {flavour} {key}: smallest margin {float(g['min_margin'].min()):.2f} = "
                          f"{float(g['min_margin'].min() / g['max_gap'].max()):.0f} x the bf16-vs-fp32 gap; faults {g['kinds']} change "
                          f"{g['faults_changed'].tolist()} of 8 frames in the copy layer, {g['other_layer_changed'].tolist()} in decoder layer {g['other_layer']}")
                if key == "bf16_b32":
                    first = g["codes"][0]
                    assert g["codes"].shape[0] == 4 and all(not torch.equal(first[i], first[j]) for i in range(first.shape[0]) for j in range(i))
        assert set(gold["cross"]) == {"decisive", "decisive_copy"} and not any(bool(c["changed"].any()) for c in gold["cross"].values())
