"""The yardstick of the endless conversations, on the oracle alone (no GPU, none of the product's code): a 16-turn conversation on csm_tiny,
flavour decisive_copy:1:20, seed 1234, 8 frames per reply, a 26-row voice prompt, 21 rows per turn.  It reaches the 248-row limit at its
12th turn and from then on drops its two oldest unpinned units before every turn.  One oracle keeps its backbone cache from turn to turn
and has it EDITED the way csm_session_forget is defined (rows below the cut untouched; later rows moved down, V as it is, K rotated back
by the rows dropped: fp32 on the bf16 values, one rounding); a second oracle runs every turn's trimmed prompt cold.

  * on every turn the edited oracle's greedy codes, the cold oracle's and ``decisive_copy_expected_codes`` of the trimmed prompt are equal
    bit for bit;
  * the smallest top-1 / top-2 margin is at least 4 x the largest logit difference between the two oracles (measured: margin 0.82, gap
    0.031, 26 x -- the test prints what it finds);
  * keys left unrotated, keys rotated by d + 1, V landing one row late, and rows not moved at all each change at least one of the first
    six frames of the turn after the first forget.

It passes without the feature: it shows that the decisive checkpoint grades it and that the expected codes are analytic."""
import torch

from test_session_forget_gpu import LAG, N, SEQ, _Policy, _news


def _rot(shape, d):
    from oracle import csm_ref as C
    s = shape.backbone
    ang = float(d) * C.llama3_scaled_rope_theta(s.head_dim, s.rope_base, s.scale_factor).double()
    return torch.cos(ang).float(), torch.sin(ang).float()


def _edit_cache(om, a, b, held, fault=None):
    """The oracle's backbone cache, rows [0, held), without its rows [a, b).  ``fault``: one of the wrong edits."""
    d = b - a
    if fault == "not_moved":
        return
    c, s = _rot(om.shape, d + 1 if fault == "rot_d_plus_1" else d)
    for k, v in zip(om.backbone.k, om.backbone.v):
        x = k[0, :, b:held].float().unflatten(-1, (-1, 2))
        x0, x1 = x[..., 0], x[..., 1]
        moved = k[0, :, b:held].clone() if fault == "unrotated" else torch.stack([x0 * c + x1 * s, x1 * c - x0 * s], dim=-1).flatten(-2).to(k.dtype)
        k[0, :, a:held - d] = moved
        late = 1 if fault == "v_one_row_late" else 0
        v[0, :, a + late:held - d + late] = v[0, :, b:held].clone()


def _run(om, full, start, n):
    """Rows [start, S) of the prompt, then n greedy frames, on the cache as it is: (codes (n, 32), logits (n, 32, V) fp32)."""
    from oracle import csm_ref as C
    t, m = full
    S = t.shape[0]
    cur_t, cur_m, pos = t[start:].unsqueeze(0), m[start:].unsqueeze(0), torch.arange(start, S).unsqueeze(0)
    codes, logits = [], []
    for _ in range(n):
        tr = C.FrameTrace()
        fr = om.generate_frame(cur_t, cur_m, pos, 1.0, 1, greedy=True, trace=tr)
        codes.append(fr[0].to(torch.int32)); logits.append(torch.stack(tr.logits)[:, 0].float())
        cur_t = torch.cat([fr.long(), torch.zeros(1, 1).long()], dim=1).unsqueeze(1)
        cur_m = torch.cat([torch.ones_like(fr).bool(), torch.zeros(1, 1).bool()], dim=1).unsqueeze(1)
        pos = pos[:, -1:] + 1
    return torch.stack(codes), torch.stack(logits)


def test_sixteen_turns_edited_cache_cold_run_and_analytic_codes_agree_and_faults_show():
    from oracle import csm_ref as C
    shape = C.csm_tiny()
    assert shape.backbone.max_seq_len == SEQ
    w = C.make_weights(shape, seed=1234, flavour=f"decisive_copy:1:{LAG}")
    warm, cold = C.OracleModel(shape, w), C.OracleModel(shape, w)
    warm.setup_caches(1); cold.setup_caches(1)
    pol, held = _Policy(), 0
    margin, gap, forgets, fault_frames = float("inf"), 0.0, 0, {}
    for k, new in enumerate(_news(1, 16, 20)):
        full, cut = pol.turn(new, N)
        S = full[0].shape[0]
        assert S < SEQ - N
        if cut:
            forgets += 1
            assert k >= 11 and cut == (26, 47) and cut[0] <= S - 1 - LAG < held - 21, "frame 0 reads a moved row"
            if not fault_frames:                               # the first forget: what each wrong edit does to this turn
                keep = [(x.clone(), y.clone()) for x, y in zip(warm.backbone.k, warm.backbone.v)]
                want = C.decisive_copy_expected_codes(shape, 1234, full[0], full[1], N, LAG)
                for fault in ("unrotated", "rot_d_plus_1", "v_one_row_late", "not_moved"):
                    _edit_cache(warm, *cut, held, fault)
                    got, _ = _run(warm, full, held - 21, N)
                    fault_frames[fault] = int((got != want).any(dim=1).sum())
                    assert bool((got[:6] != want[:6]).any()), f"the fault '{fault}' leaves the first six frames of the turn after the forget as they are"
                    for (x, y), (x0, y0) in zip(zip(warm.backbone.k, warm.backbone.v), keep):
                        x.copy_(x0); y.copy_(y0)
            _edit_cache(warm, *cut, held)
            held -= cut[1] - cut[0]
        else:
            assert k < 11
        got_w, log_w = _run(warm, full, held, N)
        cold.reset_caches()
        got_c, log_c = _run(cold, full, 0, N)
        want = C.decisive_copy_expected_codes(shape, 1234, full[0], full[1], N, LAG)
        assert torch.equal(got_w, want), f"turn {k}: the edited-cache oracle leaves the analytic codes of the trimmed prompt"
        assert torch.equal(got_c, want), f"turn {k}: the cold oracle leaves the analytic codes of the trimmed prompt"
        for lg in (log_w, log_c):
            top = lg.topk(2, dim=-1).values
            margin = min(margin, float((top[..., 0] - top[..., 1]).min()))
        gap = max(gap, float((log_w - log_c).abs().max()))
        pol.reply(full, got_w)
        held = S + N - 1                                        # every reply is cut at its limit: its last frame's row is not written
    print(f"forgets {forgets}, smallest margin {margin:.3f}, largest edited-vs-cold logit difference {gap:.4f}, ratio {margin / gap:.1f}, "
          f"frames of 8 changed by each fault {fault_frames}")
    assert forgets == 5, "turns 12..16 each drop two units"
    assert margin >= 4 * gap, f"margin {margin} < 4 x gap {gap}"
