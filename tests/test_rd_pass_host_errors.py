"""The error contract of the host twin of the second intra pass (csrc/pnn_rd_pass.cpp, the second-pass part of csrc/pnn_tskip.cpp),
pinned in the manner of tests/test_gpu_eval_errors.py: one row per refusal of each of the seven entries -- the arguments that provoke
it, the return code, everything the call wrote to stderr (captured on the file descriptor: the entries use the C library's fprintf) --
and rows with two bad arguments at once, where the entry's own order of checks decides which one is named.  The texts are written out
here, never taken from the library.

Every refusal happens before anything is written: after each refused call every output still holds its guard bytes.

The name a refusal is reported under is part of the contract, with its quirks as they stand: a call without signalling through the
_signal_ or _codec_ entries reports as pnn_rd_pass_host (the _tskip_ entry refuses such a call itself); a fault the first pass finds
inside the second pass reports as pnn_first_pass_signal_host or pnn_first_pass_codec_host, by codec; with signalling RDOQ's lambda is
checked in front of the QPs, over the indices `qps && qi < nb_qps && qi < 8` only; a refused smoothing is named by the first pass's own
line in front of the entry's.

Smallest shapes: two blocks of width 4 with the 9 x 9 patterns of tests/rd_pass_cases.py, one QP, a lambda given (so that rows can
spoil it), no neighbours; one row at width 8 (17 x 17 patterns), where transform skip is refused."""
import ctypes
import os
import tempfile

import numpy as np
import pytest

from context_adaptive_neural_network_based_prediction_amd import _lib
from tests import rd_pass_cases as cases

PNN_E_ARG = -1                       # include/pnn_hip.h
GUARD, PAD, SLOT = 0xC5, 256, 1024   # an output starts PAD bytes into its slot of guard bytes (the largest, [2][11] doubles, takes 176)
OUT = object()                       # in a template: a guarded output


class Qps(list):
    """In a template: an array of int."""


class Lambdas(list):
    """In a template: an array of double."""


# The arguments of a call that each entry accepts, in the order of its C declaration.  A string names a buffer of `env`.
BLOCKS = dict(patterns="patterns", pattern_h=9, pattern_w=9, targets="targets", width=4, n=2, cand_pred="cand", smoothing=0,
              qps=Qps([22]), nb_qps=1, lambdas=Lambdas([30.]))
NEIGHBOURS = dict(left_modes=None, above_modes=None)
RD_OUTPUTS = ("cand_modes", "cand_costs", "best_mode", "best_slot", "best_cost", "best_sse", "best_rate")
SIDE_OUTPUTS = ("first_pass_costs", "best_side_rate")
LIST_OUTPUTS = ("list_modes", "list_costs", "slot_modes")


def outs(*names):
    return {name: OUT for name in names}


def none(*names):
    return {name: None for name in names}


E_RD, E_RDOQ, E_SIGNAL, E_CODEC, E_TSKIP, E_FIRST, E_FIRST_CODEC = (
    "pnn_rd_pass_host", "pnn_rd_pass_rdoq_host", "pnn_rd_pass_signal_host", "pnn_rd_pass_codec_host", "pnn_rd_pass_tskip_host",
    "pnn_first_pass_signal_host", "pnn_first_pass_codec_host")
GOOD = {
    E_RD: dict(BLOCKS, sign_data_hiding=0, **outs(*RD_OUTPUTS)),
    E_RDOQ: dict(BLOCKS, sign_data_hiding=0, rdoq=0, **outs(*RD_OUTPUTS)),
    E_SIGNAL: dict(BLOCKS, sign_data_hiding=0, rdoq=0, signalling=1, **NEIGHBOURS, **outs(*RD_OUTPUTS, *SIDE_OUTPUTS)),
    E_CODEC: dict(BLOCKS, sign_data_hiding=0, rdoq=0, signalling=1, **NEIGHBOURS, codec=1, **outs(*RD_OUTPUTS, *SIDE_OUTPUTS)),
    E_TSKIP: dict(BLOCKS, sign_data_hiding=0, rdoq=0, signalling=1, **NEIGHBOURS, codec=0, transform_skip=1,
                  **outs(*RD_OUTPUTS, *SIDE_OUTPUTS, "best_ts_flag")),
    E_FIRST: dict(BLOCKS, **NEIGHBOURS, **outs(*LIST_OUTPUTS)),
    E_FIRST_CODEC: dict(BLOCKS, **NEIGHBOURS, codec=1, **outs(*LIST_OUTPUTS)),
}

WIDTH = "the width of the target patch is not 4, 8, 16, 32 or 64."
NEGATIVE = "negative batch size."
NO_CAND = "the candidate's predictions are NULL."
NO_OUTPUT = "every output is NULL."
QPS = "the QPs are not 1 to 8 integers in [0, 51]."
LAMBDA = "a lambda is negative or not finite."
RDOQ_LAMBDA = "RDOQ with a lambda that is not above 0."
FIRST_PASS = "the first pass refused the arguments (pattern sides, NULL inputs or smoothing)."
NEIGHBOUR = "a neighbour mode is not 0 .. %d or 255."
CODEC = "the codec is not 0 (switch) or 1 (substitution)."
SUBSTITUTION_WITHOUT = "the substitution codec without signalling: HM never searches without the mode bits."
SIDE_WITHOUT = "first_pass_costs or best_side_rate without signalling."
TS_RANGE = "transform_skip is not 0 or 1."
TS_WIDTH = "transform skip at a width other than 4."
TS_WITHOUT = "the second pass with transform skip without signalling."
TS_LAMBDA = "transform skip with a lambda that is not finite or not above 0."
SMOOTHING = "The reference-sample smoothing %d is not 0 (none), 1 (HM without StrongIntraSmoothing) or 2 (HM).\n"    # the first pass's own line
BAD_36, BAD_35 = "modes_36", "modes_35"            # neighbour arrays of `env`: block 1 has 36 (never a mode) / 35 (no mode of the substitution codec)
NINE = dict(nb_qps=9, qps=Qps([22] * 9), lambdas=Lambdas([30.] * 9))
WIDTH_8 = dict(width=8, pattern_h=17, pattern_w=17)                                  # (the buffers follow the width)


def rows_of(entry, outer, inner, outputs, changes=None, rdoq=False, top=None, own_lambda=None, own_width=None, outputs_first=False):
    """The refusals an entry shares with the others and the rows that pin their order.  `changes`: what puts the entry on this path
    (a codec, an option off).  `outer`: the name the entry's own checks report under; `inner`: the name of the checks the first pass
    runs (the same where the entry has one body).  `rdoq`: the entry has the option; `top`: with neighbours, their largest mode;
    `own_lambda`, `own_width`: the texts of a lambda check and a width check of the entry's own in front of everything here (transform
    skip on); `outputs_first`: the entry checks its outputs in front of the first pass's checks (the second pass with signalling)."""
    base = dict(changes or {})

    def row(change, name, text, before=""):
        return (entry, dict(base, **change), "%s%s: %s\n" % (before, name, text))

    bad_lambda, bad_width = (outer, own_lambda) if own_lambda else (inner, LAMBDA), own_width or WIDTH
    rows = [
        row(dict(width=12), outer, bad_width), row(dict(width=0), outer, bad_width), row(dict(n=-1), inner, NEGATIVE),
        row(none("cand_pred"), inner, NO_CAND), row(none(*outputs), outer, NO_OUTPUT),
        row(dict(nb_qps=0), inner, QPS), row(NINE, inner, QPS), row(dict(qps=Qps([52])), inner, QPS), row(dict(qps=Qps([-1])), inner, QPS),
        row(none("qps"), inner, QPS),
        row(dict(lambdas=Lambdas([-1.])), *bad_lambda), row(dict(lambdas=Lambdas([float("nan")])), *bad_lambda),
        row(dict(lambdas=Lambdas([float("inf")])), *bad_lambda),
        row(dict(pattern_h=4), inner, FIRST_PASS), row(dict(pattern_h=10), inner, FIRST_PASS), row(dict(pattern_w=4), inner, FIRST_PASS),
        row(dict(pattern_w=10), inner, FIRST_PASS), row(none("patterns"), inner, FIRST_PASS), row(none("targets"), inner, FIRST_PASS),
        row(dict(smoothing=3), inner, FIRST_PASS, SMOOTHING % 3), row(dict(smoothing=-1), inner, FIRST_PASS, SMOOTHING % -1),
        row(dict(width=12, n=-1), outer, bad_width),                                 # the width before the batch
        row(dict(none("cand_pred"), n=-1), inner, NEGATIVE),                         # the batch before the candidate
        row(dict(none("cand_pred", *outputs)), *((outer, NO_OUTPUT) if outputs_first else (inner, NO_CAND))),
        row(dict(none(*outputs), nb_qps=0), outer, NO_OUTPUT),                       # the outputs before the QPs
        row(dict(none("cand_pred"), nb_qps=0), inner, NO_CAND),                      # the candidate before the QPs
        row(dict(pattern_h=4, smoothing=3), inner, FIRST_PASS),                      # the sides before the smoothing: its line is not written
        row(dict(none("patterns"), smoothing=3), inner, FIRST_PASS)]                 # ... and so are the inputs
    if not own_lambda:
        rows += [
            row(dict(nb_qps=0, lambdas=Lambdas([-1.])), inner, QPS),                 # the QPs' count before the lambdas
            row(dict(lambdas=Lambdas([-1.]), pattern_h=4), inner, LAMBDA),           # the lambdas before the first pass's own checks
            # QP and lambda are checked index by index: the first lambda before the second QP
            row(dict(nb_qps=2, qps=Qps([22, 52]), lambdas=Lambdas([-1., 30.])), inner, LAMBDA),
            row(dict(nb_qps=2, qps=Qps([52, 22]), lambdas=Lambdas([-1., 30.])), inner, QPS)]
    if rdoq and not own_lambda:
        rows += [row(dict(rdoq=1, lambdas=Lambdas([0.])), outer, RDOQ_LAMBDA)]
    if top:
        rows += [
            row(dict(left_modes=BAD_36), inner, NEIGHBOUR % top), row(dict(above_modes=BAD_36), inner, NEIGHBOUR % top),
            row(dict(left_modes=BAD_36, pattern_h=4), inner, NEIGHBOUR % top)]       # the neighbours before the first pass's own checks
        if top == 34:
            rows += [row(dict(left_modes=BAD_35), inner, NEIGHBOUR % 34), row(dict(above_modes=BAD_35), inner, NEIGHBOUR % 34)]
        if not own_lambda:
            rows += [row(dict(lambdas=Lambdas([-1.]), left_modes=BAD_36), inner, LAMBDA)]         # the lambdas before the neighbours
    return rows


def without_signalling_rows(entry, changes=None):
    """pnn_rd_pass_rdoq_host's body, whichever entry forwards to it: everything reports as pnn_rd_pass_host."""
    name = "pnn_rd_pass_host"
    rows = rows_of(entry, name, name, RD_OUTPUTS, changes, rdoq=entry != E_RD)
    if entry != E_RD:
        base = dict(changes or {})
        rows += [
            (entry, dict(base, rdoq=1, lambdas=Lambdas([-1.])), "%s: %s\n" % (name, LAMBDA)),             # the lambda's range before RDOQ's
            (entry, dict(base, rdoq=1, lambdas=Lambdas([0.]), qps=Qps([52])), "%s: %s\n" % (name, QPS)),  # the QP before RDOQ's lambda
            (entry, dict(base, rdoq=1, lambdas=Lambdas([0.]), pattern_h=4), "%s: %s\n" % (name, RDOQ_LAMBDA)),
            (entry, dict(base, **none(*RD_OUTPUTS), rdoq=1, lambdas=Lambdas([0.])), "%s: %s\n" % (name, NO_OUTPUT))]
    return rows


def with_signalling_rows(entry, outer, codec, changes=None, own_lambda=None, own_width=None):
    """rd_pass_body behind `entry`: width, outputs and RDOQ's lambda under `outer`, everything else under the first pass's name."""
    inner = "pnn_first_pass_codec_host" if codec else "pnn_first_pass_signal_host"
    outputs = RD_OUTPUTS + SIDE_OUTPUTS + (("best_ts_flag",) if entry == E_TSKIP else ())
    rows = rows_of(entry, outer, inner, outputs, changes, rdoq=True, top=34 if codec else 35, own_lambda=own_lambda, own_width=own_width,
                   outputs_first=True)
    if own_lambda:
        return rows
    base = dict(changes or {})

    def row(change, name, text):
        return (entry, dict(base, **change), "%s: %s\n" % (name, text))

    return rows + [
        row(dict(rdoq=1, lambdas=Lambdas([-1.])), outer, RDOQ_LAMBDA), row(dict(rdoq=1, lambdas=Lambdas([float("nan")])), outer, RDOQ_LAMBDA),
        row(dict(rdoq=1, lambdas=Lambdas([float("inf")])), inner, LAMBDA),           # above 0: left to the first pass
        row(dict(none(*outputs), rdoq=1, lambdas=Lambdas([0.])), outer, NO_OUTPUT),  # the outputs before RDOQ's lambda
        row(dict(width=12, rdoq=1, lambdas=Lambdas([0.])), outer, WIDTH),
        # RDOQ's lambda in front of the QPs' own check, over the indices `qps && qi < nb_qps && qi < 8`
        row(dict(rdoq=1, lambdas=Lambdas([0.]), qps=Qps([52])), outer, RDOQ_LAMBDA),
        row(dict(rdoq=1, lambdas=Lambdas([0.]), n=-1), outer, RDOQ_LAMBDA),
        row(dict(rdoq=1, lambdas=Lambdas([0.]), qps=None), inner, QPS),
        row(dict(rdoq=1, lambdas=Lambdas([0.]), nb_qps=0), inner, QPS),
        row(dict(NINE, rdoq=1, lambdas=Lambdas([30.] * 8 + [0.])), inner, QPS),
        row(dict(NINE, rdoq=1, lambdas=Lambdas([30.] * 7 + [0., 30.])), outer, RDOQ_LAMBDA)]


def own(entry, change, text):
    return (entry, change, "%s: %s\n" % (entry, text))


SOME_BLOCK = dict(pattern_h=4)
ROWS_TABLE = (
    without_signalling_rows(E_RD) + without_signalling_rows(E_RDOQ)

    + with_signalling_rows(E_SIGNAL, E_SIGNAL, 0) + [
        own(E_SIGNAL, dict(signalling=0), SIDE_WITHOUT), own(E_SIGNAL, dict(none(SIDE_OUTPUTS[0]), signalling=0), SIDE_WITHOUT),
        own(E_SIGNAL, dict(none(SIDE_OUTPUTS[1]), signalling=0), SIDE_WITHOUT),
        own(E_SIGNAL, dict(signalling=0, width=12), SIDE_WITHOUT)]                   # ... in front of everything
    + without_signalling_rows(E_SIGNAL, dict(none(*SIDE_OUTPUTS), signalling=0))

    + with_signalling_rows(E_CODEC, E_CODEC, 1) + [
        own(E_CODEC, dict(codec=2), CODEC), own(E_CODEC, dict(codec=-1), CODEC), own(E_CODEC, dict(signalling=0), SUBSTITUTION_WITHOUT),
        own(E_CODEC, dict(none(*SIDE_OUTPUTS), signalling=0), SUBSTITUTION_WITHOUT),
        own(E_CODEC, dict(codec=2, signalling=0), CODEC),                            # the codec before the signalling
        own(E_CODEC, dict(codec=2, width=12), CODEC), own(E_CODEC, dict(signalling=0, width=12), SUBSTITUTION_WITHOUT),    # ... and both before everything
        (E_CODEC, dict(codec=0, signalling=0), "%s: %s\n" % (E_SIGNAL, SIDE_WITHOUT))]           # codec 0: the _signal_ entry, under its name
    + with_signalling_rows(E_CODEC, E_SIGNAL, 0, dict(codec=0))
    + without_signalling_rows(E_CODEC, dict(none(*SIDE_OUTPUTS), codec=0, signalling=0))

    + with_signalling_rows(E_TSKIP, E_TSKIP, 0, own_lambda=TS_LAMBDA, own_width=TS_WIDTH) + [
        own(E_TSKIP, dict(transform_skip=2), TS_RANGE), own(E_TSKIP, dict(transform_skip=-1), TS_RANGE),
        own(E_TSKIP, WIDTH_8, TS_WIDTH),
        own(E_TSKIP, dict(codec=2), CODEC), own(E_TSKIP, dict(codec=-1), CODEC),
        own(E_TSKIP, dict(signalling=0), TS_WITHOUT), own(E_TSKIP, dict(signalling=0, transform_skip=0), TS_WITHOUT),
        own(E_TSKIP, dict(none(*SIDE_OUTPUTS, "best_ts_flag"), signalling=0, transform_skip=0), TS_WITHOUT),     # (no way to the pass without signalling)
        own(E_TSKIP, dict(codec=1, signalling=0), TS_WITHOUT),
        own(E_TSKIP, dict(lambdas=Lambdas([0.])), TS_LAMBDA), own(E_TSKIP, dict(rdoq=1, lambdas=Lambdas([0.])), TS_LAMBDA),
        own(E_TSKIP, dict(transform_skip=2, **WIDTH_8), TS_RANGE),                   # the option's range before the width
        own(E_TSKIP, dict(codec=2, **WIDTH_8), TS_WIDTH),                            # the width before the codec
        own(E_TSKIP, dict(codec=2, signalling=0), CODEC),                            # the codec before the signalling
        own(E_TSKIP, dict(signalling=0, lambdas=Lambdas([0.])), TS_WITHOUT),         # the signalling before the lambda
        own(E_TSKIP, dict(SOME_BLOCK, transform_skip=2), TS_RANGE), own(E_TSKIP, dict(SOME_BLOCK, codec=2), CODEC),
        own(E_TSKIP, dict(SOME_BLOCK, signalling=0), TS_WITHOUT), own(E_TSKIP, dict(SOME_BLOCK, lambdas=Lambdas([0.])), TS_LAMBDA),
        own(E_TSKIP, dict(none(*RD_OUTPUTS, *SIDE_OUTPUTS, "best_ts_flag"), lambdas=Lambdas([0.])), TS_LAMBDA),  # the lambda before the outputs
        own(E_TSKIP, dict(width=12, lambdas=Lambdas([0.])), TS_WIDTH),
        # the option's lambda over the indices `qps && qi < nb_qps && qi < 8`, in front of the QPs' own check
        own(E_TSKIP, dict(lambdas=Lambdas([0.]), qps=Qps([52])), TS_LAMBDA),
        (E_TSKIP, dict(lambdas=Lambdas([0.]), qps=None), "pnn_first_pass_signal_host: %s\n" % QPS),
        (E_TSKIP, dict(lambdas=Lambdas([0.]), nb_qps=0), "pnn_first_pass_signal_host: %s\n" % QPS),
        (E_TSKIP, dict(NINE, lambdas=Lambdas([30.] * 8 + [0.])), "pnn_first_pass_signal_host: %s\n" % QPS),
        own(E_TSKIP, dict(NINE, lambdas=Lambdas([30.] * 7 + [0., 30.])), TS_LAMBDA),
        (E_TSKIP, dict(codec=1, left_modes=BAD_35), "pnn_first_pass_codec_host: %s\n" % (NEIGHBOUR % 34)),
        (E_TSKIP, dict(codec=1, n=-1), "pnn_first_pass_codec_host: %s\n" % NEGATIVE)]
    + with_signalling_rows(E_TSKIP, E_TSKIP, 0, dict(transform_skip=0))             # the option off: the body's own lambda checks
    + [(E_TSKIP, dict(transform_skip=0, codec=1, above_modes=BAD_35), "pnn_first_pass_codec_host: %s\n" % (NEIGHBOUR % 34)),
       own(E_TSKIP, dict(transform_skip=0, **WIDTH_8, **none(*RD_OUTPUTS, *SIDE_OUTPUTS, "best_ts_flag")), NO_OUTPUT)]

    + rows_of(E_FIRST, E_FIRST, E_FIRST, LIST_OUTPUTS, top=35)
    + rows_of(E_FIRST_CODEC, E_FIRST_CODEC, E_FIRST_CODEC, LIST_OUTPUTS, top=34) + [
        own(E_FIRST_CODEC, dict(codec=2), CODEC), own(E_FIRST_CODEC, dict(codec=-1), CODEC),
        own(E_FIRST_CODEC, dict(codec=2, width=12), CODEC)]                          # the codec before everything
    + rows_of(E_FIRST_CODEC, E_FIRST, E_FIRST, LIST_OUTPUTS, dict(codec=0), top=35))  # codec 0: the _signal_ entry, under its name


@pytest.fixture(scope="module")
def env():
    """Every input buffer, made once: the blocks by width, the neighbour arrays."""
    made = {w: dict(zip(("patterns", "targets", "cand"), cases.seeded(w, 2))) for w in (4, 8)}
    made["modes_36"], made["modes_35"] = np.array([0, 36], np.uint8), np.array([255, 35], np.uint8)
    return made


def call(env, entry, changes):
    """Calls `entry` with its accepted arguments but for `changes`; returns (rc, what the call wrote to stderr, the guard slots after
    the call)."""
    args = dict(GOOD[entry], **changes)
    assert set(args) == set(GOOD[entry]), "a row names an argument the entry does not have"
    guards = np.full((len(args), SLOT), GUARD, np.uint8)
    blocks = env[args["width"] if args["width"] in env else 4]
    keep, values = [], []
    for k, v in enumerate(args.values()):
        if v is OUT:
            v = guards[k].ctypes.data + PAD
        elif isinstance(v, Qps):
            keep.append((ctypes.c_int * len(v))(*v))
            v = keep[-1]
        elif isinstance(v, Lambdas):
            keep.append((ctypes.c_double * len(v))(*v))
            v = keep[-1]
        elif isinstance(v, str):
            v = (blocks[v] if v in blocks else env[v]).ctypes.data
        values.append(v)
    function = getattr(_lib.lib(), entry)
    libc = ctypes.CDLL(None)
    with tempfile.TemporaryFile() as log:
        libc.fflush(None)
        saved = os.dup(2)
        os.dup2(log.fileno(), 2)
        try:
            rc = function(*values)
            libc.fflush(None)
        finally:
            os.dup2(saved, 2)
            os.close(saved)
        log.seek(0)
        written = log.read().decode()
    return rc, written, guards


def row_id(row):
    return "%s-%s" % (row[0][4:], ",".join("%s=%s" % (k, "NULL" if v is None else v) for k, v in row[1].items()))


@pytest.mark.parametrize("entry, changes, written", ROWS_TABLE, ids=[row_id(r) for r in ROWS_TABLE])
def test_refusal_code_text_and_untouched_outputs(env, entry, changes, written):
    rc, got, guards = call(env, entry, changes)
    assert rc == PNN_E_ARG
    assert got == written
    assert (guards == GUARD).all(), "a refused call wrote to an output"


def test_every_refusal_of_the_table_is_distinct_and_every_entry_is_covered():
    assert len({(r[0], repr(sorted(r[1].items(), key=repr))) for r in ROWS_TABLE}) == len(ROWS_TABLE)
    assert {r[0] for r in ROWS_TABLE} == set(GOOD)


ACCEPTED = [(entry, {}) for entry in GOOD] + [
    (E_SIGNAL, dict(none(*SIDE_OUTPUTS), signalling=0)), (E_CODEC, dict(codec=0)), (E_CODEC, dict(none(*SIDE_OUTPUTS), codec=0, signalling=0)),
    (E_TSKIP, dict(transform_skip=0)), (E_TSKIP, dict(codec=1)), (E_FIRST_CODEC, dict(codec=0)),
    (E_RDOQ, dict(rdoq=1)), (E_SIGNAL, dict(rdoq=1, left_modes=BAD_35, above_modes=BAD_35))]


@pytest.mark.parametrize("entry, changes", ACCEPTED, ids=[row_id(r) for r in ACCEPTED])
def test_the_unchanged_arguments_are_accepted(env, entry, changes):
    """Each row's refusal is that of its change alone: the paths the rows start from are accepted, write nothing to stderr, and write
    to every output (so the guards above could have told) without touching the bytes in front of it."""
    rc, got, guards = call(env, entry, changes)
    assert rc == 0 and got == ""
    for k, v in enumerate(dict(GOOD[entry], **changes).values()):
        assert v is not OUT or not (guards[k] == GUARD).all()
    assert (guards[:, :PAD] == GUARD).all()
