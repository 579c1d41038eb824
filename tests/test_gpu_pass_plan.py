"""The plan of every launch path of the pass layer (csrc/pnn_passes.cpp), case by case (tests/pass_plan_cases.py): what a call launches
is part of its behaviour -- a pass that comes to disagree with itself (a K-segmented layer folded in one place and reduced in another, a
tail planned and not taken, a layer counted twice) shows here before it shows in a profile.

The triples are last_call_stats() -- (launches, gemm_launches, gemm_flops) -- of the library as it stood BEFORE the pass layer's launch
set-ups were gathered into single helpers, recorded by running this file against that build (PNN_LIB_PATH); tools/lib_ab_plan.py compares
the same cases' outputs and [pnn] lines between two builds.  The flops are sums of integers below 2^53: compared with ==.
What the counts show: conv 4 / 8 / 16 at 1 and 5 blocks = the pair launches + the first convolutions' launch, merger and last layer as
tails; conv 32 / 64 fold their K segments inside the launches (seg_fold = 0: six seg_reduce launches more); pair = 0 and time_launches = 1
go layer by layer (12 GEMM launches), the timed pass with a seg_reduce behind every segmented layer; conv 64 at 5 blocks is past the
pair path's tile cap; FC at 600 blocks adds fuse_reduce behind fc_out_f32, at 1024 the output layer rides in the third layer's launch."""
import pytest

from tests import pass_plan_cases as C

pytestmark = pytest.mark.gpu

EXPECTED = {
    "fc4_1": (4, 4, 5990400.0),
    "fc4_5": (4, 4, 29952000.0),
    "fc4_600": (5, 4, 3594240000.0),
    "fc4_1024": (4, 3, 6134169600.0),
    "fc8_1": (4, 4, 6681600.0),
    "fc8_5": (4, 4, 33408000.0),
    "fc8_600": (5, 4, 4008960000.0),
    "fc8_1024": (4, 3, 6841958400.0),
    "conv4_1": (3, 2, 1769472.0),
    "conv4_5": (3, 2, 8847360.0),
    "conv8_1": (3, 2, 7077888.0),
    "conv8_5": (3, 2, 35389440.0),
    "conv16_1": (7, 6, 95944704.0),
    "conv16_5": (7, 6, 479723520.0),
    "conv32_1": (11, 8, 541065216.0),
    "conv32_5": (11, 8, 2705326080.0),
    "conv64_1": (11, 8, 2340421632.0),
    "conv64_5": (22, 12, 11702108160.0),
    "conv16_256_twice": (13, 9, 24561844224.0),
    "fc8_1_sp": (5, 4, 6681600.0),
    "fc8_5_sp": (5, 4, 33408000.0),
    "fc8_1024_sp": (5, 3, 6841958400.0),
    "conv16_1_sp": (9, 6, 95944704.0),
    "conv16_200_sp": (11, 9, 19188940800.0),
    "conv32_1_pair0": (16, 12, 541065216.0),
    "conv32_1_tails0": (11, 8, 541065216.0),
    "conv32_1_chain_io0": (11, 8, 541065216.0),
    "conv32_1_seg_fold0": (17, 8, 541065216.0),
    "conv32_1_two_streams": (16, 12, 541065216.0),
    "conv32_1_timed": (22, 12, 541065216.0),
    "conv32_70_seq": (16, 12, 37874565120.0),
    "fc8_5_chunk3": (8, 8, 33408000.0),
    "conv16_5_chunk3": (14, 12, 479723520.0),
    "conv16_tbs_2": (7, 6, 191889408.0),
    "conv16_tbs_200": (13, 9, 19188940800.0),
    "conv16_tbs_2_sp": (10, 6, 191889408.0),
    "conv16_tbs_200_sp": (11, 9, 19188940800.0),
}


def test_every_case_has_a_triple():
    assert sorted(EXPECTED) == sorted(C.NAMES)


@pytest.mark.parametrize("case", C.CASES, ids=C.NAMES)
def test_pass_plan(case):
    _, stats = C.run_case(case)
    assert stats == EXPECTED[case[0]], "%s: (launches, gemm_launches, gemm_flops) = %r, recorded %r" % (case[0], stats, EXPECTED[case[0]])
