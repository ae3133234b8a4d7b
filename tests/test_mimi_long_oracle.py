"""tests/golden/mimi_long.pt (oracle/make_golden.py --only mimilong) checked on the CPU: it carries its seeds, its shapes fit, the oracle
reproduces its shortest clip bit for bit -- and the faults tests/test_mimi_long_gpu.py is there to see (an attention window one token
short or long, no window, a RoPE angle taken modulo the stream pool's ring) each move the oracle's compared samples by >= 10 x the 2e-5
of peak that the GPU test allows, so a codec with such a fault cannot pass it.  For the encode side: the window faults change the
codes of >= 10 % of the frames past the window, and the inputs do not sit on quantiser ties (a 1e-6 nudge of the latent leaves >= 97 %
of the frames alone), so the 10 % of near-tie frames that ``_check_codes`` tolerates is not where a fault could hide."""
import os

import pytest
import torch

from oracle import mimi_ref as M
from oracle import make_golden as G

GOLD = os.path.join(os.path.dirname(__file__), "golden")
A = G.MIMI_LONG


@pytest.fixture(scope="module")
def gold():
    return torch.load(os.path.join(GOLD, "mimi_long.pt"))


@pytest.fixture(scope="module")
def full():
    s = M.mimi_full()
    return s, M.make_weights(s, seed=A["weight_seed"], encoder=True)


def test_fixture_carries_its_seeds_and_its_shapes_fit(gold):
    assert gold["weight_seed"] == A["weight_seed"] == 4321
    assert gold["bound"] == 2e-5 and gold["fault_factor"] == 10.0 and gold["pool_ring"] == 250 + 2 * 10
    assert [(g["frames"], g["code_seed"]) for g in gold["decode"]] == list(A["decode"])
    assert [f for f, _ in A["decode"]] == [126, 150, 300, 1125]
    assert 0 < gold["longest_oracle_seconds"] <= 60, "the longest clip is one the oracle decodes in about a minute"
    for g in gold["decode"]:
        T = g["frames"]
        codes = G.mimi_long_codes(g["code_seed"], T)
        assert codes.shape == (1, 32, T) and int((codes[0] * torch.arange(1, T + 1)).sum()) == g["code_checksum"]
        assert g["pcm_stride16"].shape == (1, 1, 1920 * T // 16) and g["pcm_stride16"].dtype == torch.float32
        assert g["pcm_head"].shape == g["pcm_tail"].shape == (1, 1, gold["window"])
        assert torch.equal(g["pcm_head"][..., ::16], g["pcm_stride16"][..., :gold["window"] // 16])
        assert torch.equal(g["pcm_tail"][..., ::16], g["pcm_stride16"][..., -gold["window"] // 16:])
    assert [(e["samples"], e["wav_seed"]) for e in gold["encode"]] == list(A["encode"]) == [(1920 * 126 + 777, 7126), (1920 * 260 + 5, 7260)]
    for e in gold["encode"]:
        T = -(-e["samples"] // 1920)
        assert e["codes"].shape == (1, 32, T) and 0 <= int(e["codes"].min()) and int(e["codes"].max()) < 2048
        assert e["frames_past_window"] == T - 125
    assert os.path.getsize(os.path.join(GOLD, "mimi_long.pt")) < 972121, "larger than the largest fixture committed before it"


def test_oracle_reproduces_the_shortest_clip_bit_for_bit(gold, full):
    s, w = full
    g = gold["decode"][0]
    assert g["frames"] == 126
    v = G.mimi_long_views(M.decode(s, w, G.mimi_long_codes(g["code_seed"], 126)))
    for name in ("stride16", "head", "tail"):
        assert torch.equal(v[name], g[f"pcm_{name}"]), name


def test_recorded_fault_margins_are_ten_times_the_bound(gold, full):
    need = gold["fault_factor"] * gold["bound"]
    assert need == pytest.approx(2e-4)
    seen = set()
    for g in gold["decode"]:
        assert set(g["fault_moves"]) == {f for f, _ in G.MIMI_LONG_FAULTS}
        for fault, move in g["fault_moves"].items():
            if G.mimi_long_fault_applies(fault, 2 * g["frames"]):
                seen.add(fault)
                assert move >= need, f"{g['frames']} frames, {fault}: {move:.3g} of peak < {need:.3g}"
            else:
                assert move == 0.0 and fault == "rope_mod_ring" and g["frames"] == 126      # 252 tokens never reach row 270
    assert seen == {f for f, _ in G.MIMI_LONG_FAULTS}
    # and one of the stored numbers is what the oracle gives today: the smallest clip, the window one token short
    s, w = full
    g = gold["decode"][0]
    codes = G.mimi_long_codes(g["code_seed"], 126)
    move = G.mimi_long_move(M.decode(s, w, codes, context=249), M.decode(s, w, codes))
    assert move == pytest.approx(g["fault_moves"]["ctx249"], rel=1e-3) and move >= need


def test_window_faults_change_the_prompts_codes_and_the_inputs_sit_on_no_ties(gold, full):
    G.mimi_long_check_encode_faults(gold["encode"])
    long_prompt = gold["encode"][1]
    assert long_prompt["frames_past_window"] == 136
    assert all(n >= 14 for n in long_prompt["frames_changed"].values())
    for e in gold["encode"]:
        assert e["tie_unchanged"] >= A["tie_unchanged_min"] == 0.97
    # the prompts the GPU test grades against the live oracle alone, and the 5 s golden prompt once more
    s, w = full
    e = gold["encode"][0]
    cases = [(e["samples"], e["wav_seed"], 1), (*A["encode_b2"], 2)] + [(n, seed, 1) for n, seed in A["encode_edges"]]
    for n, seed, rows in cases:
        z = M.encode_latent(s, w, G.mimi_long_wav(seed, n, rows))
        assert z.shape == (rows, 512, -(-n // 1920))
        codes = M.quantize(s, w, z)
        unchanged = G.mimi_long_tie_unchanged(s, w, z, codes, seed)
        assert unchanged >= A["tie_unchanged_min"], f"{n} samples: {unchanged:.3f} of the frames survive the nudge"
    assert torch.equal(codes, M.encode(s, w, G.mimi_long_wav(seed, n, rows))), "quantize(encode_latent) is encode"
    assert torch.equal(M.quantize(s, w, M.encode_latent(s, w, G.mimi_long_wav(e["wav_seed"], e["samples"]))), e["codes"].long())


def test_the_oracles_fault_arguments_default_to_the_model():
    s = M.mimi_tiny()
    w = M.make_weights(s, seed=4321, encoder=True)
    codes = torch.randint(0, 2048, (1, 32, 9), generator=torch.Generator().manual_seed(3))
    pcm = M.decode(s, w, codes)
    assert torch.equal(pcm, M.decode(s, w, codes, context=s.tr_context, rope_mod=1 << 20))
    assert not torch.equal(pcm, M.decode(s, w, codes, context=s.tr_context - 1))
    assert not torch.equal(pcm, M.decode(s, w, codes, context=M.NO_WINDOW))
    assert not torch.equal(pcm, M.decode(s, w, codes, rope_mod=s.tr_context + 2))
    wav = torch.randn(1, 1, 1920 * 8 + 11, generator=torch.Generator().manual_seed(4)) * 0.3
    z = M.encode_latent(s, w, wav)
    assert torch.equal(z, M.encode_latent(s, w, wav, context=s.tr_context, rope_mod=1 << 20))
    assert not torch.equal(z, M.encode_latent(s, w, wav, context=s.tr_context + 1))
