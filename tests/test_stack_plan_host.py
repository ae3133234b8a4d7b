"""The launch plan of a transformer layer (sesameai-tts_amd/csrc/stack_plan.h: no HIP) as a stand-alone host program.  The wide-M kernel
families are bit-identical to one another, so the parity tests cannot see a call that takes another kernel than it did; the program pins
which family, split and activation order every listed call chooses, and which public ``kind`` numbers ``csm_op_gemv`` accepts."""
from host_check import build_and_run


def test_stack_plan_under_the_host_sanitizers(tmp_path):
    build_and_run("stack_plan_check", tmp_path)
