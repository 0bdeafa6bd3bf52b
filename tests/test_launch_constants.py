"""The thresholds that the shapes of tests/test_launch_shapes.py rest on, read from the sources.

Those tests reach a launch path by choosing a shape on either side of a constant (4096 pods,
1024 and 4096 metric columns, 16 cards).  If someone moves a constant, the shapes would pass
on without reaching their branch; this test fails instead.  No GPU."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "platform-aware-scheduling_amd", "csrc")
HINT = "move the shapes of tests/test_launch_shapes.py with it"


def _source(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def _constant(src, name):
    m = re.search(rf"constexpr\s+int\s+{name}\s*=\s*(\d+)\s*;", src)
    assert m, f"tas_eval.hip no longer defines {name} as a plain integer: {HINT}"
    return int(m.group(1))


def test_grouping_thresholds():
    src = _source("tas_eval.hip")
    for name, want in (("kGroupTpb", 1024), ("kGU", 4), ("kMaxGroupMetrics", 4096)):
        got = _constant(src, name)
        assert got == want, f"tas_eval.hip: {name} is {got}, was {want}: {HINT}"
    # the single-round condition of group_body, the refusal and the LDS limit of the prep
    for text in ("g.P <= kGroupTpb * kGU && g.M <= kGroupTpb", "M > kMaxGroupMetrics",
                 "group_lds > 64 * 1024"):
        assert text in src, f"tas_eval.hip no longer holds `{text}`: {HINT}"
    # the per-call knobs of the global-pass path
    for knob in ("PAS_EVAL_GLOBAL_PASS", "PAS_EVAL_GPASS_PODS"):
        assert f'env_int("{knob}", 0)' in src, f"tas_eval.hip no longer reads {knob}: {HINT}"


def test_topk_card_tiers():
    src = _source("tas_gas_topk.hip")
    m = re.search(r"void topk_dispatch\(.*?\n}\n", src, re.S)
    assert m, f"tas_gas_topk.hip: topk_dispatch not found: {HINT}"
    tiers = [int(x) for x in re.findall(r"if \(a\.K <= (\d+)\)", m.group(0))]
    assert tiers == [8, 16], f"tas_gas_topk.hip: topk_dispatch tiers on a.K are {tiers}: {HINT}"
    assert "tas_gas_topk_kernel<PAS_GAS_MAX_CARDS, kMaxRes, kWide, kAfter>" in m.group(0), HINT


def test_narrow_limit_shapes():
    """tests/test_narrow_limits.py: pods of <= 32 and of 33..40 rules on either side of
    kStageRules, 1 / 4 / 6 rules on the prioritize metric around kSkip, requests of 70 rules
    past one kRuleTile."""
    hint = "move the shapes of tests/test_narrow_limits.py with it"
    topk, req = _source("tas_gas_topk.hip"), _source("tas_request_batch.hip")
    for src, name, want in ((topk, "kPodLanes", 32), (topk, "kSkip", 4), (req, "kRuleTile", 64)):
        m = re.search(rf"constexpr\s+int\s+{name}\s*=\s*(\d+)\s*;", src)
        assert m, f"{name} is no longer a plain integer: {hint}"
        assert int(m.group(1)) == want, f"{name} is {m.group(1)}, was {want}: {hint}"
    # kStageRules is the pod's lane count, and the staging decision a ballot over the wave
    for text in ("constexpr int kStageRules = kPodLanes;",
                 "!__ballot(have && r1 - r0 > kStageRules)",
                 "t0 < r1; t0 += kRuleTile"):
        assert text in topk + req, f"the sources no longer hold `{text}`: {hint}"
