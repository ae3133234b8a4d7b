"""Host logic of the group refill (no GPU): a scripted model stands in for the frame loop and records its calls.  What is checked is the
scheduling of ``_BesideTheLoop`` with ``group > 1`` (sesameai/live_batch.py): which slots one begin call takes, that everything a refill needs
-- prefix copies grouped by handle, then the per-slot sampling calls -- sits in front of the ONE ``refill_group_begin`` with no frame step in
between, that a group never carries more than ``max_prefill_rows`` rows, that the per-step budget counts the group's rows together -- and
that ``group=1`` is exactly today's call list."""
import pytest
import torch

from test_host_logic import _FakeCodec
from test_prefix_host_logic import VOICE_A, VOICE_B, _Beside, _prompts, _rows, _scripts


class _Group(_Beside):
    """``_Beside`` plus the group surface of sesameai.models.Model: a group needs 16 layers of work like a single refill, all its slots are
    parked until it completes and emit their frame 0 in the step after."""
    max_prefill_rows = 1 << 20

    def reset_caches(self):
        super().reset_caches()
        self.group_pending = None

    def refill_begin(self, slot, tokens, mask, **kw):
        assert self.group_pending is None, "one refill OR one group"
        super().refill_begin(slot, tokens, mask, **kw)

    def refill_group_begin(self, slots, prompts, starts=None):
        assert self.pending is None and self.group_pending is None, "one refill OR one group"
        rows = [int(t.shape[0]) for t, _ in prompts]
        assert len(set(slots)) == len(slots) == len(prompts) == len(starts) and sum(rows) <= self.max_prefill_rows
        self.log.append(("group_begin", list(slots), [int(t[-1, 32]) for t, _ in prompts], rows, list(starts)))
        self.group_pending = [[(s, int(t[-1, 32])) for s, (t, _) in zip(slots, prompts)], 16]
        for s in slots:
            self.cur[s] = None

    def refill_group_advance(self, k):
        self.log.append(("group_advance", k))
        self.group_pending[1] -= k
        if self.group_pending[1] > 0:
            return False
        for s, pid in self.group_pending[0]:
            self.cur[s] = [pid, 0, True]
        self.group_pending = None
        return True

    def set_slot_sampling(self, slots, T, k, seed=None):
        self.log.append(("sampling", list(slots), seed))

    def clear_slot_sampling(self, slots=None):
        self.log.append(("clear", list(slots)))


def _gen(model, slots, budget):
    from sesameai.generator import Generator
    gen = Generator(model, audio_tokenizer=_FakeCodec(), max_batch_size=slots)
    gen.refill_row_layers = budget
    return gen


def test_four_vacated_slots_take_four_prompts_in_one_begin():
    lens = [5, 5, 5, 5, 12, 12, 9, 3, 7, 4, 6]               # six slots: the first four end in the same block, two keep generating
    scripts = _scripts(lens, 11)
    model = _Group(scripts, 6)
    gen = _gen(model, 6, 40)
    ha, hb = gen.cache_prefix(*_rows(VOICE_A)), gen.cache_prefix(*_rows(VOICE_B))
    del model.log[:]
    prompts, match = _prompts(len(lens))
    seeds = [None if i % 3 == 0 else 50 + i for i in range(len(lens))]
    out = gen.generate_codes_continuous(prompts, 12, 0.9, 50, seed=seeds, refill_group=4)
    for i, n in enumerate(lens):
        assert torch.equal(out[i], scripts[i][: min(n, 12)].to(torch.int32)), f"request {i}"
    log = model.log
    assert not [e for e in log if e[0] in ("refill_begin", "advance")], "with a group size every refill is a group call"
    begins = [k for k, e in enumerate(log) if e[0] == "group_begin"]
    assert [log[k][2] for k in begins] == [[0, 1, 2, 3], [4, 5], [6, 7, 8, 9], [10]], "initial fill (4 + 2), the four vacated slots together, the last prompt"
    assert sorted(log[begins[2]][1]) == [0, 1, 2, 3]
    assert not [e for e in log[:begins[1]] if e[0] == "step"], "the initial fill: no frame step before every slot has its prompt"
    for k in begins:
        _, slots, ids, rows, starts = log[k]
        assert starts == [match[i] for i in ids] and rows == [prompts[i][0].shape[0] - match[i] for i in ids], "only the rows after each match run"
        j = k
        while j > 0 and log[j - 1][0] in ("apply", "sampling", "clear"):
            j -= 1
        head = log[j:k]                                         # what sits between the last step / advance and this begin
        assert j == 0 or log[j - 1][0] in ("step", "group_advance")
        kinds = [e[0] for e in head]
        n_apply = kinds.count("apply")
        assert kinds[:n_apply] == ["apply"] * n_apply and "apply" not in kinds[n_apply:], "the copies first, then the sampling calls"
        copied = {}
        for _, h, sl in head[:n_apply]:
            assert h not in copied, "one copy per handle"
            copied[h] = sl
        if k not in begins[:2]:                                 # (the initial fill's copies are the scheduler's shared ones, made before)
            want = {}
            for s, i in zip(slots, ids):
                if match[i]:
                    want.setdefault(0 if i % 2 == 0 else 1, []).append(s)
            assert copied == want
        seeded = [e[1][0] for e in head if e[0] == "sampling"]
        assert seeded == [s for s, i in zip(slots, ids) if seeds[i] is not None], "every seeded request's entry, in the order of the group"
    # the budget counts the group's rows together: the first advance after the vacated slots' begin, with nobody left waiting
    k = begins[2]
    adv = next(e for e in log[k + 1:] if e[0] == "group_advance")
    assert adv[1] == max(1, min(40 * 1 // sum(log[k][3]), 16))
    gen.drop_prefix(ha); gen.drop_prefix(hb)


def test_a_group_never_exceeds_max_prefill_rows():
    lens = [4, 4, 4, 4, 6, 6, 6, 6, 3]
    scripts = _scripts(lens, 12)
    model = _Group(scripts, 4)
    model.max_prefill_rows = 70                                # whole prompts of 23 / 15 / 23 / 15 / 4 ... rows: three fit, the fourth waits
    gen = _gen(model, 4, 40)
    prompts, _ = _prompts(len(lens))
    out = gen.generate_codes_continuous(prompts, 12, 0.9, 50, refill_group=4)
    for i, n in enumerate(lens):
        assert torch.equal(out[i], scripts[i][: min(n, 12)].to(torch.int32)), f"request {i}"
    groups = [e for e in model.log if e[0] == "group_begin"]
    assert all(sum(e[3]) <= 70 for e in groups)
    assert groups[0][2] == [0, 1, 2] and groups[1][2][0] == 3, "the prompt that did not fit opens the next group"
    assert sorted(i for e in groups for i in e[2]) == list(range(len(lens)))


def test_group_of_one_is_todays_call_list():
    lens = [3, 9, 0, 5, 14, 2, 7]
    logs = []
    for kw in ({}, {"refill_group": 1}):
        model = _Group(_scripts(lens, 3), 3)
        gen = _gen(model, 3, 40)
        ha = gen.cache_prefix(*_rows(VOICE_A))
        prompts, _ = _prompts(len(lens))
        gen.generate_codes_continuous(prompts, 12, 0.9, 50, seed=[None, 5, None, 6, None, None, 7], **kw)
        logs.append(list(model.log))
        gen.drop_prefix(ha)
    assert logs[0] == logs[1] and not [e for e in logs[1] if e[0].startswith("group")]
    with pytest.raises(ValueError):
        gen.generate_codes_continuous(prompts, 12, 0.9, 50, refill_group=0)


def test_argument_checks_under_the_host_sanitizers(tmp_path):
    """csm_refill_group_begin's validation and table construction (csrc/rag_segs.h: no HIP) as a stand-alone host program built with
    AddressSanitizer and UBSan: every refusal input of the C ABI, the accepted tables, sums at the edge of int."""
    import os
    import shutil
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hipcc = shutil.which("hipcc") or os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "bin", "hipcc")
    exe = str(tmp_path / "refill_group_args_check")
    r = subprocess.run([hipcc, "-std=c++17", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all",
                        "-I", os.path.join(root, "sesameai-tts_amd", "csrc"), os.path.join(root, "tools", "refill_group_args_check.cpp"), "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok" and "runtime error" not in r.stderr, r.stdout + r.stderr
