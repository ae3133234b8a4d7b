"""CPU side of the norm-test checkpoints (oracle.csm_ref.norm_test_weights: RMSNorm scales != 1) and their golden
`csm1b_norms.pt` (oracle/make_golden.py --only norms; tests/test_norms_gpu.py holds the HIP path to it): the checkpoints are what
they claim to be, the golden carries the seeds and prompts it was made from, and every scale fault it stores moves the logits by
more than the tests' tolerance -- a regenerated golden cannot quietly lose its teeth."""
import os

import torch

GOLD = os.path.join(os.path.dirname(__file__), "golden")


def _scales(w):
    return [k for k in w if k.endswith(".scale")]


def test_norm_test_weights_are_deterministic_jittered_and_have_outlier_channels():
    from oracle import csm_ref as C
    shape = C.csm_tiny()
    j, j2 = C.norm_test_weights(shape), C.norm_test_weights(shape)
    o, o2 = C.norm_test_weights(shape, outliers=True), C.norm_test_weights(shape, outliers=True)
    base = C.make_weights(shape, seed=1234, norm_jitter=0.2)
    assert all(torch.equal(j[k], j2[k]) and torch.equal(j[k], base[k]) for k in base)
    assert all(torch.equal(o[k], o2[k]) for k in o)
    ow = C.with_norm_outliers(shape, j, 1234)
    assert all(torch.equal(o[k], ow[k]) for k in o)
    names = _scales(j)
    assert len(names) == 2 * (shape.backbone.num_layers + shape.decoder.num_layers) + 2
    for k in base:
        if k not in names:
            assert torch.equal(o[k], j[k]), f"{k}: the outlier variant changed a matrix"
    for k in names:
        js, os_ = j[k].float(), o[k].float()
        assert 0.17 < float(js.std()) < 0.23, f"{k}: jitter std {float(js.std()):.3f}"
        assert abs(float(js.mean()) - 1.0) < 0.05
        big = os_.abs() >= C.NORM_OUTLIER_LO * js.abs()
        assert int(big.sum()) >= C.NORM_OUTLIERS, f"{k}: {int(big.sum())} outlier channels"
        assert int((os_ != js).sum()) <= C.NORM_OUTLIERS
        assert bool((os_.abs() <= C.NORM_OUTLIER_HI * js.abs() * 1.01).all())


def test_norm_faults_edit_only_what_they_name():
    from oracle import csm_ref as C
    shape = C.csm_tiny()
    w = C.norm_test_weights(shape)
    for fault in C.NORM_FAULTS:
        f = C.norm_fault_weights(shape, w, fault)
        changed = [k for k in w if not torch.equal(w[k], f[k])]
        assert changed and all(k.endswith(".scale") for k in changed), (fault, changed)
        for k in changed:
            if fault.endswith("_one"):
                assert bool((f[k] == 1).all())
            else:
                assert torch.equal(torch.sort(w[k].float())[0], torch.sort(f[k].float())[0]) or fault == "dec2_swap"
    assert len([k for k in w if not torch.equal(w[k], C.norm_fault_weights(shape, w, "dec2_swap")[k])]) == 2
    p = C.norm_fault_weights(shape, w, "bb7_sa_pieces")
    name = f"backbone.layers.{shape.backbone.num_layers - 1}.sa_norm.scale"
    assert torch.equal(p[name][:8], w[name][8:16]) and torch.equal(p[name][8:16], w[name][:8])


def test_norms_golden_carries_its_seeds_and_prompts():
    import bench
    from types import SimpleNamespace
    from oracle import csm_ref as C
    from oracle.make_golden import NORMS_LEGS, norms_prompt
    gold = torch.load(os.path.join(GOLD, "csm1b_norms.pt"))
    shape = C.csm_1b()
    assert int(gold["weight_seed"]) == 1234
    args = SimpleNamespace(ctx_text=40, ctx_frames=125, gen_text=24)
    bt, bm = bench.synthetic_prompt(args, 1, shape.text_vocab_size, seed0=int(gold["prompts"]["cfg2"]["seed"]))
    tok, msk = norms_prompt(shape, "cfg2")
    assert torch.equal(bt[0], tok) and torch.equal(bm[0], msk), "the config-2 prompt is not bench.py's"
    g5 = torch.load(os.path.join(GOLD, "csm1b_cfg5.pt"))["s1334"]
    tok5, msk5 = norms_prompt(shape, "cfg5")
    assert torch.equal(g5["prompt_tokens"].long(), tok5) and torch.equal(g5["prompt_mask"], msk5), "the config-5 prompt is not csm1b_cfg5.pt's"
    for name, (t, m) in (("cfg2", (tok, msk)), ("cfg5", (tok5, msk5))):
        assert torch.equal(gold["prompt_checksum"][name], torch.stack([t.sum(), m.sum(), torch.tensor(t.shape[0])])), name
    for leg, variant, dtype, pname, n in NORMS_LEGS:
        g = gold["legs"][leg]
        assert (g["checkpoint"], g["weights"], g["prompt"], int(g["rows"])) == (variant, dtype, pname, norms_prompt(shape, pname)[0].shape[0])
        assert g["codes"].shape == (n, 32) and g["top_v"].shape == (n, 32, 8) and g["top_i"].shape == (n, 32, 8)
        assert g["margin"].shape == (n, 32) and g["bf16_vs_fp32_gap"].shape == (n, 32)
        assert bool((g["bf16_vs_fp32_gap"] > 0).all())
        assert ("deq_checksum" in g) == (dtype == "fp8")
    assert os.path.getsize(os.path.join(GOLD, "csm1b_norms.pt")) < 300 * 1024


def test_every_stored_norm_fault_moves_the_logits_by_at_least_one_and_a_half_gaps():
    from oracle import csm_ref as C
    from oracle.make_golden import NORMS_FAULT_LEGS, NORMS_FAULT_MIN
    gold = torch.load(os.path.join(GOLD, "csm1b_norms.pt"))
    assert NORMS_FAULT_MIN >= 1.5
    kept = set()
    for leg in NORMS_FAULT_LEGS:
        g = gold["legs"][leg]
        gap = float(g["bf16_vs_fp32_gap"].max())
        for fault, d in g["faults"].items():
            assert fault in C.NORM_FAULTS
            assert float(d) >= 1.5 * gap, f"leg {leg} {fault}: {float(d):.4f} < 1.5 x gap {gap:.4f}"
            kept.add(fault)
    assert all(f in gold["legs"]["A"]["faults"] for f in ("scales_one", "dec2_swap", "dec_final_one")), "leg A lost a fault"
    assert "dec2_swap" in gold["legs"]["A"]["faults"], "the GPU mutation check needs leg A's dec2_swap"
    assert kept == set(C.NORM_FAULTS), f"faults that clear 1.5 x gap on no leg: {set(C.NORM_FAULTS) - kept}"
