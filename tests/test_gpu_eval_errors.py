"""The error contract of the evaluator's C-ABI entries (csrc/pnn_eval.cpp), pinned: one row per refusal of each entry -- the
arguments that provoke it, the return code and the exact pnn_last_error text -- and rows with two bad arguments at once, where an
entry's own order of checks decides which one is named.  The texts are the format strings of the entries as they stood when each
got its own copy of the checks; they are written out here, never taken from the library.

Every refusal happens before any launch: after each refused call every output still holds its guard bytes.  Smallest shapes that
reach every check: w = 4, one picture of 16 x 20 (it holds the 12 x 12 contexts and the 16 x 16 IPFCN-S lines with room to step one
pixel outside), two positions, a seeded FC-4 net and a seeded width-4 IPFCN-S in one context, and a context that holds neither.

The entries of the second intra pass that have a body of their own (the _rdoq_, _signal_, _codec_ with a codec other than 0 and
_tskip_ entries, dense and on picture pairs) are in the table with one QP; w = 4 is the width at which transform skip is legal.  For
them an accepted call precedes every refused one: the launch count it left must survive the refusal, and the scratch stays untouched."""
import ctypes

import numpy as np
import pytest

from context_adaptive_neural_network_based_prediction_amd import _lib
from context_adaptive_neural_network_based_prediction_amd import ipfcns as I
from tests import util
from tests.util import dev, stream

pytestmark = pytest.mark.gpu

PNN_E_ARG = -1                       # include/pnn_hip.h
W, H_PIC, W_PIC = 4, 16, 20
ROWS, COLS = [0, 4], [0, 8]                        # contexts: the near corner and the far one (16 - 12, 20 - 12)
LINE_ROWS, LINE_COLS = [0, 0], [0, 4]              # IPFCN-S line origins: the only row (16 - 16), the two end columns
GUARD, PAD, SLOT = 0xC5, 256, 1024                 # an output starts PAD bytes into its slot of guard bytes (the largest, [2][35] uint32, takes 280)
OUT, STREAM, BYTES = object(), object(), object()  # in a template: a guarded output / the current stream / the scratch's byte count


class Qps(list):
    """In a template: a host array of int."""


class Lambdas(list):
    """In a template: a host array of double."""


class Workspace:
    """In a template: the scratch, as large as the entry's own *_workspace_bytes function asks for; BYTES then passes that count minus
    `short`.  `offset` moves the pointer (to misalign it)."""
    def __init__(self, short=0, offset=0):
        self.short, self.offset = short, offset

    def __repr__(self):
        return "Workspace(short=%d, offset=%d)" % (self.short, self.offset)


# The arguments of a call that each entry accepts, in the order of its C declaration.  A string names a buffer of `env`.
PICTURE = dict(images=1, height=H_PIC, width_ch=W_PIC, d_rows=ROWS, d_cols=COLS, positions=2)
SCORES = dict(mask_w=0, mask_h=0, d_targets=OUT, d_pnn_u8=OUT, d_pnn_f32=OUT, d_pnn_sse=OUT, d_hevc_mode=OUT, d_hevc_sse=OUT,
              d_hevc_pred=OUT, stream=STREAM)
HADS = dict(d_cand_pred="cand", d_mode_hads=OUT, d_cand_hads=OUT, d_list_modes=OUT, d_list_costs=OUT, stream=STREAM)
DENSE = dict(c="full", width=W, d_patterns="patterns", pattern_h=9, pattern_w=9, d_targets="targets", n=2)
GOOD = {
    "pnn_hevc_best_mode_device": dict(DENSE, d_best_mode=OUT, d_best_sse=OUT, d_best_pred=OUT, d_mode_sse=OUT, stream=STREAM),
    "pnn_hevc_mode_hads_device": dict(DENSE, **HADS),
    "pnn_ipfcns_load": dict(c="full", width=W, params="ipfcns_params", n_floats=I.n_params(W)),
    "pnn_ipfcns_forward_device": dict(c="full", width=W, d_x="x", n=2, d_out_f32=OUT, stream=STREAM),
    "pnn_ipfcns_predict_device": dict(dict(c="full", width=W, d_channels="decoded", **PICTURE), d_rows=LINE_ROWS, d_cols=LINE_COLS,
                                      d_targets="targets", d_pred_u8=OUT, d_pred_f32=OUT, d_means=OUT, d_sse=OUT, stream=STREAM),
    "pnn_score_pictures_device": dict(c="full", width=W, d_channels="decoded", **PICTURE, **SCORES),
    "pnn_score_picture_pairs_device": dict(c="full", width=W, d_context_channels="decoded", d_target_channels="original", **PICTURE, **SCORES),
    "pnn_first_pass_picture_pairs_device": dict(c="full", width=W, d_context_channels="decoded", d_target_channels="original", **PICTURE,
                                                mask_w=0, mask_h=0, **HADS),
    "pnn_score_f32_device": dict(c="full", width=W, d_pred_f32="pred_f32", d_channels="decoded", **PICTURE, d_pred_u8=OUT, d_sse=OUT,
                                 stream=STREAM),
}

E_BEST, E_HADS, E_LOAD, E_FWD, E_PRED, E_PIC, E_PAIR, E_FIRST, E_F32 = GOOD

# The second intra pass.  One QP, a lambda given (so that rows can spoil it), no neighbours; the _codec_ entries with the substitution
# codec (with 0 they forward), the _tskip_ entries with the option on and the flag output.
PAIR = dict(c="full", width=W, d_context_channels="decoded", d_target_channels="original", **PICTURE, mask_w=0, mask_h=0)
RD = dict(d_cand_pred="cand", smoothing=0, qps=Qps([22]), nb_qps=1, lambdas=Lambdas([30.]), sign_data_hiding=0, rdoq=0)
SIGNAL = dict(signalling=1, d_left_modes=None, d_above_modes=None)
RD_OUTPUTS = ("d_cand_modes", "d_cand_costs", "d_best_mode", "d_best_slot", "d_best_cost", "d_best_sse", "d_best_rate")
SIDE_OUTPUTS = ("d_first_pass_costs", "d_best_side_rate")
TAIL = dict(d_workspace=Workspace(), workspace_bytes=BYTES, stream=STREAM)


def outs(*names):
    return {name: OUT for name in names}


for blocks, suffix in ((DENSE, "_device"), (PAIR, "_picture_pairs_device")):
    GOOD.update({
        "pnn_rd_pass_rdoq" + suffix: dict(blocks, **RD, **outs(*RD_OUTPUTS), **TAIL),
        "pnn_rd_pass_signal" + suffix: dict(blocks, **RD, **SIGNAL, **outs(*RD_OUTPUTS, *SIDE_OUTPUTS), **TAIL),
        "pnn_rd_pass_codec" + suffix: dict(blocks, **RD, **SIGNAL, codec=1, **outs(*RD_OUTPUTS, *SIDE_OUTPUTS), **TAIL),
        "pnn_rd_pass_tskip" + suffix: dict(blocks, **RD, **SIGNAL, codec=0, transform_skip=1,
                                           **outs(*RD_OUTPUTS, *SIDE_OUTPUTS, "d_best_ts_flag"), **TAIL)})
SECOND_PASS = [entry for entry in GOOD if entry.startswith("pnn_rd_pass_")]
# what an accepted call of the table launches: 4 without signalling, 2 + 3 nb_qps with it, 2 + 7 nb_qps with transform skip and the flag
LAUNCHES = {entry: 4 if "_rdoq_" in entry else 9 if "_tskip_" in entry else 5 for entry in SECOND_PASS}
# the entry's own size function and which of the call's arguments it takes behind (width, n, nb_qps)
SIZE_FUNCTION = {"rdoq": ("pnn_rd_pass_workspace_bytes", ()), "signal": ("pnn_rd_pass_signal_workspace_bytes", ("signalling",)),
                 "codec": ("pnn_rd_pass_codec_workspace_bytes", ("signalling", "codec")),
                 "tskip": ("pnn_rd_pass_tskip_workspace_bytes", ("signalling", "codec", "transform_skip"))}

BAD_WIDTH = "width 12 is not 4, 8, 16, 32 or 64"
NO_IPFCNS_WIDTH = "no IPFCN-S for width 64 (4, 8, 16 or 32)"
NO_IPFCNS_LOADED = "no IPFCN-S loaded for width %d"
SIDES = "intra pattern %dx%d: both sides must lie in [5, 9]"
MASKS = "masks (%d, %d): both must belong to {0, 4, ..., 4}"
DENSE_INPUTS = "bad batch size or input buffers"
NEGATIVE = "negative sizes"
TOO_MANY = "more than 2^31 - 1 blocks"
NO_OUTPUT = "every output is NULL"
NO_INPUT = "NULL input buffers"
ONE_PLANE = "one plane of the pair is NULL (%s)"
NEEDS_CAND = "d_cand_hads needs d_cand_pred"
NEEDS_TARGETS = "d_sse needs d_targets"
NO_MODEL = "a PNN output is asked for, but no model is loaded for width 4"
POSITION = "position 1 (%d, %d): the 12x12 context leaves the 16x20 picture"
SHRUNK = "position 1 (4, 8): the 12x12 context leaves the %dx%d picture"     # the far context, the picture one pixel short
LINE_ORIGIN = "line origin 1 (%d, %d): the 16x16 lines leave the 16x20 picture"
NULL_CONTEXT = None                                # pins the code only: there is no context to ask for the text
HUGE = dict(images=65536, positions=32768)         # 2^31 blocks: refused on the product, before anything is read


def none(*names):
    return {name: None for name in names}


def dense_rows(entry, outputs):
    return [(entry, dict(c=None), NULL_CONTEXT), (entry, dict(width=12), BAD_WIDTH),
            (entry, dict(pattern_h=4), SIDES % (4, 9)), (entry, dict(pattern_h=10), SIDES % (10, 9)),
            (entry, dict(pattern_w=4), SIDES % (9, 4)), (entry, dict(pattern_w=10), SIDES % (9, 10)),
            (entry, dict(n=-1), DENSE_INPUTS), (entry, none("d_patterns"), DENSE_INPUTS), (entry, none("d_targets"), DENSE_INPUTS),
            (entry, none(*outputs), NO_OUTPUT),
            (entry, dict(width=12, pattern_h=4), BAD_WIDTH),                         # the width before the sides
            (entry, dict(pattern_w=10, n=-1), SIDES % (9, 10)),                      # the sides before the batch
            (entry, dict(none(*outputs), n=-1), DENSE_INPUTS)]                       # the batch before the outputs


def picture_rows(entry):
    """The checks that the three entries on (pairs of) pictures with masks share, in their order."""
    return [(entry, dict(c=None), NULL_CONTEXT), (entry, dict(width=12), BAD_WIDTH), (entry, dict(width=0), "width 0 is not 4, 8, 16, 32 or 64"),
            (entry, dict(mask_w=2), MASKS % (2, 0)), (entry, dict(mask_h=6), MASKS % (0, 6)),          # no multiples of 4
            (entry, dict(mask_w=8), MASKS % (8, 0)), (entry, dict(mask_h=8), MASKS % (0, 8)),          # above w
            (entry, dict(mask_w=-4), MASKS % (-4, 0)),
            (entry, dict(images=-1), NEGATIVE), (entry, dict(positions=-1), NEGATIVE), (entry, dict(height=-1), NEGATIVE),
            (entry, dict(width_ch=-1), NEGATIVE), (entry, HUGE, TOO_MANY),
            (entry, none("d_rows"), NO_INPUT), (entry, none("d_cols"), NO_INPUT),
            (entry, dict(d_rows=[0, 5]), POSITION % (5, 8)), (entry, dict(d_cols=[0, 9]), POSITION % (4, 9)),
            (entry, dict(d_rows=[0, -1]), POSITION % (-1, 8)), (entry, dict(d_cols=[0, -1]), POSITION % (4, -1)),
            (entry, dict(height=15), SHRUNK % (15, 20)), (entry, dict(width_ch=19), SHRUNK % (16, 19)),
            (entry, dict(width=12, mask_w=2), BAD_WIDTH),                            # the width before the masks
            (entry, dict(mask_w=2, images=-1), MASKS % (2, 0)),                      # the masks before the sizes
            (entry, dict(d_rows=[0, 5], d_cols=None), NO_INPUT)]                     # the buffers before the positions


def pair_rows(entry, outputs):
    planes = ("d_context_channels", "d_target_channels")
    return picture_rows(entry) + [
        (entry, none(planes[0]), ONE_PLANE % planes[0]), (entry, none(planes[1]), ONE_PLANE % planes[1]),
        (entry, dict(none(planes[0]), images=0), ONE_PLANE % planes[0]),             # ... also of an empty call
        (entry, none(*planes), NO_INPUT),                                            # no plane at all is no pair: an input is missing
        (entry, none(*outputs), NO_OUTPUT),
        (entry, dict(none(planes[1]), width=12), ONE_PLANE % planes[1]),             # the pair before the width
        (entry, dict(none(*outputs), height=-1), NEGATIVE),                          # the sizes before the outputs
        (entry, dict(none(*outputs), **HUGE), NO_OUTPUT)]                            # the outputs before the block count


SMOOTHING = "smoothing %d is not 0 (none), 1 ([1 2 1]) or 2 (HM: strong allowed)"
NO_CAND = "d_cand_pred is NULL"
TOO_MANY_SLOTS = "more than 2^31 - 1 candidate slots"
QPS = "the QPs are not 1 to 8 integers in [0, 51]"
LAMBDA = "lambda 0 is negative or not finite"
RDOQ_LAMBDA = "RDOQ with lambda 0 not finite or not above 0"
WS_NULL = "d_workspace is NULL or not aligned to 8 bytes"
WS_SHORT = "the workspace has %%(have)d bytes, %s asks for %%(need)d"       # the test fills in what it passed and what the size function said
NEIGHBOUR = "%s neighbour mode %d of block 1 is not 0 .. %d or 255"
SIDE_WITHOUT = "d_first_pass_costs or d_best_side_rate without signalling"
CODEC = "codec %d is not 0 (switch) or 1 (substitution)"
SUBSTITUTION_WITHOUT = "the substitution codec without signalling"
TS_RANGE = "transform_skip %d is not in 0 .. 1"
TS_WIDTH = "transform skip at width %d (4 only)"
TS_WITHOUT = "the second pass with transform skip without signalling"
BAD_36, BAD_35 = "modes_36", "modes_35"            # neighbour arrays of `env`: block 1 has 36 (never a mode) / 35 (no mode of the substitution codec)


def second_pass_rows(entry):
    """The refusals of one entry of the second intra pass and the rows that pin its order of checks."""
    pairs, rung = "picture_pairs" in entry, entry.split("_")[3]
    signalling, tskip = rung != "rdoq", rung == "tskip"
    outputs = RD_OUTPUTS + (SIDE_OUTPUTS if signalling else ()) + (("d_best_ts_flag",) if tskip else ())
    short = WS_SHORT % {"rdoq": "pnn_rd_pass_workspace_bytes", "signal": "pnn_rd_pass_signal_workspace_bytes",
                        "codec": "pnn_rd_pass_codec_workspace_bytes", "tskip": "pnn_rd_pass_tskip_workspace_bytes"}[rung]
    # with transform skip on, the decision's lambda is checked like RDOQ's, in front of the pass's own lambda check
    bad_lambda = RDOQ_LAMBDA if tskip else LAMBDA
    if pairs:
        planes = ("d_context_channels", "d_target_channels")
        blocks = picture_rows(entry) + [
            (entry, none(planes[0]), ONE_PLANE % planes[0]), (entry, none(planes[1]), ONE_PLANE % planes[1]),
            (entry, dict(none(planes[0]), images=0), ONE_PLANE % planes[0]),
            (entry, none(*planes), NO_INPUT),                                        # no pair: the last check of all finds the input missing
            (entry, dict(none(planes[1]), width=12), ONE_PLANE % planes[1]),         # the pair before the width
            (entry, dict(height=-1, smoothing=3), NEGATIVE),                         # the blocks before the smoothing
            (entry, dict(smoothing=3, **HUGE), SMOOTHING % 3),                       # the smoothing before the block count
            (entry, dict(none("d_cand_pred"), **HUGE), TOO_MANY),                    # the block count before the candidate
            (entry, dict(none(*outputs), **HUGE), TOO_MANY),                         # ... and before the outputs
            (entry, none(*outputs), NO_OUTPUT)]
    else:
        blocks = dense_rows(entry, outputs) + [
            # refused on the product, before anything is read (with transform skip on, the dense entry's early size test would speak first)
            (entry, dict(n=0x7fffffff, **(dict(transform_skip=0) if tskip else {})), TOO_MANY_SLOTS),
            (entry, dict(n=-1, smoothing=3), DENSE_INPUTS)]                          # the blocks before the smoothing
    if tskip:       # at a width other than 4 the option is refused first: the width's own rows are those of the option off
        blocks = [(e, dict(changes, transform_skip=0) if "width" in changes else changes, text) for e, changes, text in blocks]
    rows = blocks + [
        (entry, dict(smoothing=3), SMOOTHING % 3), (entry, dict(smoothing=-1), SMOOTHING % -1),
        (entry, none("d_cand_pred"), NO_CAND),
        (entry, dict(nb_qps=0), QPS), (entry, dict(nb_qps=9), QPS), (entry, dict(qps=Qps([52])), QPS), (entry, dict(qps=Qps([-1])), QPS),
        (entry, none("qps"), QPS),
        (entry, dict(lambdas=Lambdas([-1.])), bad_lambda), (entry, dict(lambdas=Lambdas([float("nan")])), bad_lambda),
        (entry, dict(lambdas=Lambdas([float("inf")])), bad_lambda),
        (entry, dict(rdoq=1, lambdas=Lambdas([0.])), RDOQ_LAMBDA),
        (entry, none("d_workspace"), WS_NULL), (entry, dict(d_workspace=Workspace(offset=4)), WS_NULL),
        (entry, dict(d_workspace=Workspace(short=1)), short),
        (entry, dict(smoothing=3, d_cand_pred=None), SMOOTHING % 3),                 # the smoothing before the candidate
        (entry, dict(d_cand_pred=None, nb_qps=0), NO_CAND),                          # the candidate before the QPs
        (entry, dict(nb_qps=0, lambdas=Lambdas([-1.])), QPS),                        # the QPs before the lambdas
        (entry, dict(none(*outputs), lambdas=Lambdas([-1.])), bad_lambda),           # the lambdas before the outputs
        (entry, dict(none(*outputs), d_workspace=None), NO_OUTPUT),                  # the outputs before the scratch
        (entry, dict(d_workspace=Workspace(short=1, offset=4)), short if tskip else WS_NULL)]   # its pointer before its size (_tskip_: see below)
    if not signalling:
        return rows + [
            (entry, dict(rdoq=1, lambdas=Lambdas([-1.])), LAMBDA),
            (entry, dict(rdoq=1, lambdas=Lambdas([0.]), d_workspace=None), WS_NULL),                 # RDOQ's lambda behind the scratch
            (entry, dict(rdoq=1, lambdas=Lambdas([0.]), d_workspace=Workspace(short=1)), short),
            (entry, dict(none(*outputs), rdoq=1, lambdas=Lambdas([0.])), NO_OUTPUT)]
    top = 34 if rung == "codec" else 35
    rows += [
        (entry, dict(d_left_modes=BAD_36), NEIGHBOUR % ("left", 36, top)), (entry, dict(d_above_modes=BAD_36), NEIGHBOUR % ("above", 36, top)),
        (entry, dict(d_left_modes=BAD_36, d_above_modes=BAD_36), NEIGHBOUR % ("left", 36, top)),
        (entry, dict(rdoq=1, lambdas=Lambdas([-1.])), bad_lambda),
        (entry, dict(none(*outputs), rdoq=1, lambdas=Lambdas([0.])), RDOQ_LAMBDA),   # RDOQ's lambda before the outputs
        (entry, dict(d_workspace=None, d_left_modes=BAD_36), WS_NULL),               # the scratch before the neighbours
        (entry, dict(d_workspace=Workspace(short=1), d_above_modes=BAD_36), short)]
    if pairs:
        rows += [(entry, dict(d_left_modes=BAD_36, d_rows=[0, 5]), NEIGHBOUR % ("left", 36, top)),       # the neighbours before the positions
                 (entry, dict(d_above_modes=BAD_36, d_cols=None), NEIGHBOUR % ("above", 36, top))]
    some_block = dict(none("d_target_channels")) if pairs else dict(pattern_h=4)     # the first refusal of the blocks
    some_block_text = ONE_PLANE % "d_target_channels" if pairs else SIDES % (4, 9)
    if rung == "signal":
        rd_short = WS_SHORT % "pnn_rd_pass_workspace_bytes"
        rows += [
            (entry, dict(signalling=0), SIDE_WITHOUT), (entry, dict(none(SIDE_OUTPUTS[0]), signalling=0), SIDE_WITHOUT),
            (entry, dict(some_block, signalling=0), SIDE_WITHOUT),                   # ... in front of everything
            # without signalling and its outputs: the _rdoq_ entry's checks, its scratch
            (entry, dict(none(*SIDE_OUTPUTS), signalling=0, d_workspace=Workspace(short=1)), rd_short),
            (entry, dict(none(*SIDE_OUTPUTS), signalling=0, rdoq=1, lambdas=Lambdas([0.]), d_workspace=None), WS_NULL),
            (entry, dict(none(*SIDE_OUTPUTS), signalling=0, d_left_modes=BAD_36, width=12), BAD_WIDTH)]
    if rung == "codec":
        rows += [
            (entry, dict(codec=2), CODEC % 2), (entry, dict(codec=-1), CODEC % -1), (entry, dict(signalling=0), SUBSTITUTION_WITHOUT),
            (entry, dict(codec=2, signalling=0), CODEC % 2),
            (entry, dict(some_block, codec=2), CODEC % 2), (entry, dict(some_block, signalling=0), SUBSTITUTION_WITHOUT),   # the codec before everything
            (entry, dict(codec=2, width=12), CODEC % 2),
            (entry, dict(d_left_modes=BAD_35), NEIGHBOUR % ("left", 35, 34)), (entry, dict(d_above_modes=BAD_35), NEIGHBOUR % ("above", 35, 34))]
    if tskip:
        switch_short, codec_short = WS_SHORT % "pnn_rd_pass_signal_workspace_bytes", WS_SHORT % "pnn_rd_pass_codec_workspace_bytes"
        rows += [
            (entry, dict(transform_skip=2), TS_RANGE % 2), (entry, dict(transform_skip=-1), TS_RANGE % -1),
            (entry, dict(width=8), TS_WIDTH % 8), (entry, dict(width=12), TS_WIDTH % 12),
            (entry, dict(codec=2), CODEC % 2), (entry, dict(codec=1, signalling=0), SUBSTITUTION_WITHOUT),
            (entry, dict(signalling=0), TS_WITHOUT), (entry, dict(signalling=0, transform_skip=0), TS_WITHOUT),
            (entry, dict(none(*SIDE_OUTPUTS), signalling=0, transform_skip=0), TS_WITHOUT),
            (entry, dict(lambdas=Lambdas([0.])), RDOQ_LAMBDA),
            (entry, dict(lambdas=Lambdas([-1.]), transform_skip=0), LAMBDA),
            (entry, dict(codec=1, d_left_modes=BAD_35), NEIGHBOUR % ("left", 35, 34)),
            (entry, dict(codec=1, transform_skip=0, d_above_modes=BAD_35), NEIGHBOUR % ("above", 35, 34)),
            (entry, dict(transform_skip=2, codec=2), TS_RANGE % 2),                  # the option before the codec
            (entry, dict(transform_skip=2, width=8), TS_RANGE % 2),                  # its range before the width
            (entry, dict(codec=2, signalling=0), CODEC % 2),                         # the codec before the signalling
            (entry, dict(some_block, transform_skip=2), TS_RANGE % 2),               # option and codec before the blocks, dense or pairs
            (entry, dict(some_block, codec=2), CODEC % 2),
            (entry, dict(signalling=0, lambdas=Lambdas([0.])), TS_WITHOUT),          # the signalling before the lambda
            (entry, dict(lambdas=Lambdas([0.]), d_workspace=Workspace(short=1)), RDOQ_LAMBDA),       # the lambda before the short scratch
            (entry, dict(lambdas=Lambdas([0.]), d_cand_pred=None), RDOQ_LAMBDA),     # ... and both before the candidate
            (entry, dict(d_workspace=Workspace(short=1), d_cand_pred=None), short),
            # The dense entry runs signalling, lambda and short scratch BEFORE its blocks, the pairs entry BEHIND geometry, smoothing and
            # block count: the same two bad arguments, the other refusal.
            (entry, dict(some_block, signalling=0), some_block_text if pairs else TS_WITHOUT),
            (entry, dict(lambdas=Lambdas([0.]), smoothing=3), SMOOTHING % 3 if pairs else RDOQ_LAMBDA),
            (entry, dict(d_workspace=Workspace(short=1), **(dict(mask_w=2) if pairs else dict(pattern_w=10))),
             MASKS % (2, 0) if pairs else short),
            # The scratch's texts: short with the option on names this rung's size function; off, the rung's below, by codec; a NULL or
            # misaligned scratch is left to the later check, whose size test then never runs.
            (entry, dict(transform_skip=0, d_workspace=Workspace(short=1)), switch_short),
            (entry, dict(transform_skip=0, codec=1, d_workspace=Workspace(short=1)), codec_short),
            (entry, dict(codec=1, d_workspace=Workspace(short=1)), short),
            (entry, dict(transform_skip=0, d_workspace=Workspace(short=1, offset=4)), WS_NULL)]
        if pairs:
            rows += [(entry, dict(signalling=0, **HUGE), TOO_MANY), (entry, dict(transform_skip=2, **HUGE), TS_RANGE % 2)]
    return rows


SCORE_OUTPUTS = ("d_targets", "d_pnn_u8", "d_pnn_f32", "d_pnn_sse", "d_hevc_mode", "d_hevc_sse", "d_hevc_pred")
HADS_OUTPUTS = ("d_mode_hads", "d_cand_hads", "d_list_modes", "d_list_costs")
ROWS_TABLE = (
    dense_rows(E_BEST, ("d_best_mode", "d_best_sse", "d_best_pred", "d_mode_sse"))
    + dense_rows(E_HADS, HADS_OUTPUTS) + [
        (E_HADS, none("d_cand_pred"), NEEDS_CAND),
        (E_HADS, none("d_cand_pred", "d_mode_hads", "d_list_modes", "d_list_costs"), NEEDS_CAND),
        (E_HADS, none("d_cand_pred", *HADS_OUTPUTS), NO_OUTPUT),                     # the outputs before the candidate

        (E_LOAD, dict(c=None), NULL_CONTEXT), (E_LOAD, dict(width=64), NO_IPFCNS_WIDTH),
        (E_LOAD, dict(width=5), "no IPFCN-S for width 5 (4, 8, 16 or 32)"), (E_LOAD, none("params"), "NULL parameters"),
        (E_LOAD, dict(width=64, params=None), NO_IPFCNS_WIDTH),
        (E_LOAD, dict(n_floats=I.n_params(W) - 1), "%d parameters given, the width-4 IPFCN-S needs %d" % (I.n_params(W) - 1, I.n_params(W))),

        (E_FWD, dict(c=None), NULL_CONTEXT), (E_FWD, dict(width=64), NO_IPFCNS_WIDTH), (E_FWD, dict(width=8), NO_IPFCNS_LOADED % 8),
        (E_FWD, dict(c="bare"), NO_IPFCNS_LOADED % 4),
        (E_FWD, dict(n=-1), "bad batch size or buffers"), (E_FWD, none("d_x"), "bad batch size or buffers"),
        (E_FWD, none("d_out_f32"), "bad batch size or buffers"), (E_FWD, dict(width=8, n=-1), NO_IPFCNS_LOADED % 8),

        (E_PRED, dict(c=None), NULL_CONTEXT), (E_PRED, dict(width=64), NO_IPFCNS_WIDTH), (E_PRED, dict(width=16), NO_IPFCNS_LOADED % 16),
        (E_PRED, dict(c="bare"), NO_IPFCNS_LOADED % 4),
        (E_PRED, dict(images=-1), NEGATIVE), (E_PRED, dict(positions=-1), NEGATIVE), (E_PRED, dict(height=-1), NEGATIVE),
        (E_PRED, dict(width_ch=-1), NEGATIVE), (E_PRED, none("d_targets"), NEEDS_TARGETS), (E_PRED, HUGE, TOO_MANY),
        (E_PRED, none("d_channels"), NO_INPUT), (E_PRED, none("d_rows"), NO_INPUT), (E_PRED, none("d_cols"), NO_INPUT),
        (E_PRED, dict(d_rows=[0, 1]), LINE_ORIGIN % (1, 4)), (E_PRED, dict(d_cols=[0, 5]), LINE_ORIGIN % (0, 5)),
        (E_PRED, dict(d_rows=[0, -1]), LINE_ORIGIN % (-1, 4)), (E_PRED, dict(d_cols=[0, -1]), LINE_ORIGIN % (0, -1)),
        (E_PRED, dict(height=15), "line origin 0 (0, 0): the 16x16 lines leave the 15x20 picture"),
        (E_PRED, dict(width_ch=19), "line origin 1 (0, 4): the 16x16 lines leave the 16x19 picture"),
        (E_PRED, dict(width=16, height=-1), NO_IPFCNS_LOADED % 16),                  # the net before the sizes
        (E_PRED, dict(height=-1, d_targets=None), NEGATIVE),                         # the sizes before the missing target
        (E_PRED, dict(none("d_targets"), **HUGE), NEEDS_TARGETS),                    # the target before the block count
        (E_PRED, dict(none("d_channels"), d_rows=[0, 1]), NO_INPUT)]

    + picture_rows(E_PIC) + [
        (E_PIC, none("d_channels"), NO_INPUT), (E_PIC, none(*SCORE_OUTPUTS), NO_OUTPUT),
        (E_PIC, dict(c="bare"), NO_MODEL), (E_PIC, dict(none(*SCORE_OUTPUTS[:3]), c="bare"), NO_MODEL)]
    + pair_rows(E_PAIR, SCORE_OUTPUTS) + [
        (E_PAIR, dict(c="bare"), NO_MODEL), (E_PAIR, dict(none(*SCORE_OUTPUTS[:3]), c="bare"), NO_MODEL),     # the SSE alone is a PNN output
        (E_PAIR, dict(c="bare", **HUGE), NO_MODEL)]                                  # the model before the block count
    + pair_rows(E_FIRST, HADS_OUTPUTS) + [
        (E_FIRST, none("d_cand_pred"), NEEDS_CAND),
        (E_FIRST, none("d_cand_pred", *HADS_OUTPUTS), NO_OUTPUT),                    # the outputs before the candidate
        (E_FIRST, dict(none("d_cand_pred"), **HUGE), NEEDS_CAND)]                    # the candidate before the block count
    + [
        (E_F32, dict(c=None), NULL_CONTEXT), (E_F32, dict(width=12), BAD_WIDTH),
        (E_F32, dict(images=-1), NEGATIVE), (E_F32, dict(positions=-1), NEGATIVE), (E_F32, dict(height=-1), NEGATIVE),
        (E_F32, dict(width_ch=-1), NEGATIVE), (E_F32, none("d_pred_u8", "d_sse"), NO_OUTPUT), (E_F32, HUGE, TOO_MANY),
        (E_F32, none("d_pred_f32"), NO_INPUT), (E_F32, none("d_channels"), NO_INPUT), (E_F32, none("d_rows"), NO_INPUT),
        (E_F32, none("d_cols"), NO_INPUT),
        (E_F32, dict(d_rows=[0, 5]), POSITION % (5, 8)), (E_F32, dict(d_cols=[0, 9]), POSITION % (4, 9)),
        (E_F32, dict(d_rows=[0, -1]), POSITION % (-1, 8)), (E_F32, dict(height=15), SHRUNK % (15, 20)),
        (E_F32, dict(width=12, images=-1), BAD_WIDTH),                               # the width before the sizes
        (E_F32, dict(none("d_pred_u8", "d_sse"), height=-1), NEGATIVE),              # the sizes before the outputs
        (E_F32, dict(none("d_pred_u8", "d_sse"), **HUGE), NO_OUTPUT),                # the outputs before the block count
        (E_F32, dict(none("d_pred_f32"), d_cols=[0, 9]), NO_INPUT)]
    + [row for entry in SECOND_PASS for row in second_pass_rows(entry)])


@pytest.fixture(scope="module")
def env():
    """The two contexts and every input buffer, made once."""
    L = _lib.lib()
    pair = util.picture_pairs(1, W, 900)[:, :H_PIC, :W_PIC]                          # (17 x 21 cut to) 16 x 20
    assert pair.shape == (1, H_PIC, W_PIC, 2)
    rng = np.random.default_rng(901)
    net = util.make_params(W, True, seed=902, out_gain=util.out_gain(W, True))
    ipfcns_params = util.ipfcns_params(W, 903)
    made = {}
    for name in ("full", "bare"):
        made[name] = ctypes.c_void_p()
        _lib.check(L.pnn_create_empty(ctypes.byref(made[name]), ctypes.c_float(util.MEAN), 0))
    _lib.check(L.pnn_load_model_params(made["full"], W, 1, net.ctypes.data_as(_lib.f32p), net.size), made["full"])
    _lib.check(L.pnn_ipfcns_load(made["full"], W, ipfcns_params.ctypes.data_as(_lib.f32p), ipfcns_params.size), made["full"])
    made.update(original=dev(pair[..., 0]), decoded=dev(pair[..., 1]), ipfcns_params=ipfcns_params,
                patterns=dev(rng.integers(0, 256, (2, 9, 9)).astype(np.uint8)), targets=dev(rng.integers(0, 256, (2, W, W)).astype(np.uint8)),
                cand=dev(rng.integers(0, 256, (2, W, W)).astype(np.uint8)), pred_f32=dev(rng.uniform(-100, 100, (2, W, W)).astype(np.float32)),
                x=dev(rng.normal(0, 40, (2, I.input_size(W))).astype(np.float32)),
                modes_36=dev(np.array([0, 36], np.uint8)), modes_35=dev(np.array([255, 35], np.uint8)))
    yield made
    for name in ("full", "bare"):
        L.pnn_destroy(made[name])


def call(env, entry, changes):
    """Calls `entry` with its accepted arguments but for `changes`; returns (rc, the context, the guard slots after the call, the
    scratch: None, or the byte count passed, the count the entry's size function gave, and the scratch's bytes after the call)."""
    import torch
    args = dict(GOOD[entry], **changes)
    assert set(args) == set(GOOD[entry]), "a row names an argument the entry does not have"
    guards = torch.full((len(args), SLOT), GUARD, dtype=torch.uint8, device="cuda")
    keep, values, scratch = [], [], None
    for k, (name, v) in enumerate(args.items()):
        if v is OUT:
            v = guards[k].data_ptr() + PAD
        elif v is STREAM:
            v = stream()
        elif isinstance(v, Qps):
            keep.append((ctypes.c_int * len(v))(*v))
            v = keep[-1]
        elif isinstance(v, Lambdas):
            keep.append((ctypes.c_double * len(v))(*v))
            v = keep[-1]
        elif isinstance(v, Workspace) or v is BYTES:
            if scratch is None:                                                       # sized for the table's shapes and this call's options
                function, options = SIZE_FUNCTION[entry.split("_")[3]]
                need = getattr(_lib.lib(), function)(W, 2, 1, *[args[o] for o in options])
                at = args["d_workspace"] or Workspace()
                scratch = [need - at.short, need, torch.full((need + 16,), GUARD, dtype=torch.uint8, device="cuda")]     # (never short in fact)
            v = scratch[0] if v is BYTES else scratch[2].data_ptr() + v.offset
        elif isinstance(v, list):
            keep.append(dev(np.asarray(v, np.int32)))
            v = keep[-1].data_ptr()
        elif isinstance(v, str) and name != "c":
            v = env[v].ctypes.data_as(_lib.f32p) if isinstance(env[v], np.ndarray) else env[v].data_ptr()
        values.append(v)
    ctx = env[args["c"]] if args["c"] else None
    values[0] = ctx
    rc = getattr(_lib.lib(), entry)(*values)
    torch.cuda.synchronize()
    if scratch:
        scratch[2] = scratch[2].cpu().numpy()
    return rc, ctx, guards.cpu().numpy(), scratch


def launches(env):
    count = ctypes.c_int(-1)
    assert _lib.lib().pnn_last_call_stats(env["full"], None, None, ctypes.byref(count)) == 0
    return count.value


def row_id(row):
    return "%s-%s" % (row[0][4:].replace("_device", ""), ",".join("%s=%s" % (k, "NULL" if v is None else v) for k, v in row[1].items()))


@pytest.mark.parametrize("entry, changes, text", ROWS_TABLE, ids=[row_id(r) for r in ROWS_TABLE])
def test_refusal_code_text_and_untouched_outputs(env, entry, changes, text):
    L = _lib.lib()
    if entry in SECOND_PASS:                                                         # an accepted call first: its launches are counted
        assert call(env, entry, {})[0] == 0 and launches(env) == LAUNCHES[entry]
    for ctx in (env["full"], env["bare"]):                                           # a text seen below was written by this call
        assert L.pnn_set_option(ctx, b"no such option", 0) == PNN_E_ARG and L.pnn_last_error(ctx) == b"unknown option no such option"
    rc, ctx, guards, scratch = call(env, entry, changes)
    assert rc == PNN_E_ARG
    if text is not NULL_CONTEXT:
        if scratch and "%(have)d" in text:
            text = text % dict(have=scratch[0], need=scratch[1])
        assert L.pnn_last_error(ctx).decode() == text
    assert (guards == GUARD).all(), "a refused call wrote to an output"
    if entry in SECOND_PASS:
        assert (scratch[2] == GUARD).all(), "a refused call wrote to the scratch"
        assert launches(env) == LAUNCHES[entry], "a refused call reset or counted launches"


def test_every_refusal_of_the_table_is_distinct_and_every_entry_is_covered():
    assert len({(r[0], repr(sorted(r[1].items()))) for r in ROWS_TABLE}) == len(ROWS_TABLE)
    assert {r[0] for r in ROWS_TABLE} == set(GOOD)


@pytest.mark.parametrize("entry", list(GOOD))
def test_the_unchanged_arguments_are_accepted(env, entry):
    """Each row's refusal is that of its change alone; and an accepted call writes (so the guards above could have told)."""
    rc, ctx, guards, scratch = call(env, entry, {})
    assert rc == 0, _lib.lib().pnn_last_error(ctx)
    assert entry == "pnn_ipfcns_load" or not (guards == GUARD).all()
    if entry in SECOND_PASS:
        assert launches(env) == LAUNCHES[entry] and not (scratch[2] == GUARD).all()
        assert (guards[:, :PAD] == GUARD).all() and (scratch[2][scratch[1]:] == GUARD).all()     # nothing in front of an output or behind the scratch
