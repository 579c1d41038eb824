"""tests/service_driver.py proved on the CPU, before a GPU is spent on it: the same drive() that tests/test_gpu_service.py runs against
the production server (pnn_service_run_table) runs here against the same C server loop in its production thread layout
($PNN_SERVICE_WORKERS=5: five width workers, four I/O threads -- what tests/tsan_service.cpp uses) with the bit-exact CPU model of the
f32 summation order (oracle/pnn_order.c) as its backend.  Every answer must be the model's for that block alone; a backend that is
wrong the way a mis-staged batch would be (rows rotated) must make the same comparison fail.
"""
import numpy as np
import pytest

from context_adaptive_neural_network_based_prediction_amd import service
from tests import service_driver as SD
from tests import util

# a fifth of the GPU load: the Python backend is called once per batch, and sets the model's layer tables up every time
COUNTS = {4: 120, 8: 120, 16: 48, 32: 24, 64: 12}
SEEDS = {4: 704, 8: 708, 16: 716, 32: 732, 64: 764}


@pytest.fixture(scope="module")
def load(oracle):
    params = {w: util.make_params(w, SD.is_fc(w), SEEDS[w], out_gain=util.out_gain(w, SD.is_fc(w))) for w in SD.WIDTHS}
    requests = SD.make_requests(counts=COUNTS, seed=770)
    want = {w: model(oracle, params, w, *requests[w]) for w in SD.WIDTHS}
    return params, requests, want, {w: oracle.epilogue(want[w], util.MEAN) for w in SD.WIDTHS}


def model(oracle, params, w, above, left):
    """The order model on stacked inputs as the service hands them to a backend.  It computes block after block, each from its own
    inputs alone (pnn_order.c: the loop over b), so row i of a batch is the model on block i alone -- checked below."""
    if left is None:
        return oracle.order_fc_forward(params[w], w, above)
    return oracle.order_conv_forward(params[w], w, above.reshape(-1, w, 3 * w), left.reshape(-1, 2 * w, w))


def model_backend(oracle, params):
    def backend(width, above, left):
        f32 = model(oracle, params, width, above, left)
        return oracle.epilogue(f32, util.MEAN), f32
    return backend


def check(res, requests, want_f32, want_pel, kinds=(SD.PEL, SD.F32)):
    """What both service tests ask of a finished run: nobody hung, no error reply, every block answered, every answer the model's."""
    assert not res.hung, "client hung: %s" % res.hung
    assert not res.errors, res.errors[:5]
    n = sum(len(requests[w][0]) for w in requests)
    assert len(res.answers) == n and res.asked == n
    assert {k[2] for k in res.answers} == set(kinds), "the load must carry every result kind"
    bad = SD.mismatches(res, want_f32, want_pel)
    assert not bad, "%d answers differ from the model on that block alone, first (width, block, kind, ask): %s" % (len(bad), bad[:5])


def test_a_batch_row_of_the_model_is_the_block_alone(oracle, load):
    params, requests, want, _ = load
    for w in SD.WIDTHS:
        above, left = requests[w]
        for i in (0, len(above) - 1):
            alone = model(oracle, params, w, above[i:i + 1], None if left is None else left[i:i + 1])
            assert np.array_equal(alone[0], want[w][i]), (w, i)


def test_the_plan_covers_every_block_once_and_every_width_per_client(load):
    _, requests, _, _ = load
    plans = SD.plan(requests, 12, (SD.PEL, SD.F32), seed=1)
    asked = sorted((w, i) for p in plans for w, i, _ in p)
    assert asked == sorted((w, i) for w in SD.WIDTHS for i in range(COUNTS[w]))
    for p in plans:
        assert {w for w, _, _ in p} == set(SD.WIDTHS)
        assert {k for _, _, k in p} == {SD.PEL, SD.F32}
    assert plans == SD.plan(requests, 12, (SD.PEL, SD.F32), seed=1) and plans != SD.plan(requests, 12, (SD.PEL, SD.F32), seed=2)
    twice = SD.plan(requests, 3, (SD.PEL, SD.F32), seed=1, asks=2)
    for p in twice:
        for a, b in zip(p[0::2], p[1::2]):
            assert a[:2] == b[:2] and b[2] == SD.OTHER[a[2]]


@pytest.mark.parametrize("shm", ["1", "0"], ids=["slots", "socket"])
def test_production_thread_layout_answers_the_order_model(oracle, load, sock_dir, monkeypatch, shm):
    """12 clients, five widths, Pel and float mixed, against five width workers and four I/O threads: every answer = the model on
    that block alone, over the shared-memory slots and over the socket protocol."""
    params, requests, want, want_pel = load
    monkeypatch.setenv("PNN_SERVICE_WORKERS", "5")
    monkeypatch.setenv("PNN_SERVICE_SHM", shm)
    monkeypatch.setenv("PNN_CACHE_MB", "0")
    monkeypatch.setenv("PNN_SERVICE_TAG", oracle.order_tag())
    sock = str(sock_dir / "pnn.sock")
    srv = service.serve_in_thread(sock, backend=model_backend(oracle, params), max_batch=256, window_us=0)
    res = SD.drive(sock, requests, 12, with_tags=True, stop_on=lambda w, i, kind, got: not np.array_equal(got, (want_pel if kind == SD.PEL else want)[w][i]))
    stats = srv.stop(timeout=60)
    check(res, requests, want, want_pel)
    assert srv.rc == 0 and stats["requests"] == sum(COUNTS.values()) and stats["clients"] == 12
    assert stats["backend_calls"] < stats["requests"] and stats["largest_batch"] >= 2      # the Python backend is slow: requests pile up behind it
    assert res.tags == {k: {w: oracle.order_tag() for w in SD.WIDTHS} for k in range(12)}
    assert res.cache == {k: (0, 0) for k in range(12)}


def test_a_backend_that_mixes_rows_fails_the_comparison(oracle, load, sock_dir, monkeypatch):
    """The negative control: Pel blocks rotated by one row of the batch and float predictions by two (a client gets the Pel answer of
    its neighbour and the float answer of another one) -- what a wrong staging offset or a mis-routed slot would do."""
    params, requests, want, want_pel = load
    right = model_backend(oracle, params)

    def wrong(width, above, left):
        pel, f32 = right(width, above, left)
        return np.roll(pel, 1, axis=0), np.roll(f32, 2, axis=0)

    monkeypatch.setenv("PNN_SERVICE_WORKERS", "5")
    monkeypatch.setenv("PNN_CACHE_MB", "0")
    sock = str(sock_dir / "pnn.sock")
    srv = service.serve_in_thread(sock, backend=wrong, max_batch=256, window_us=2000)
    res = SD.drive(sock, requests, 12)
    stats = srv.stop(timeout=60)
    assert not res.hung and not res.errors and stats["largest_batch"] >= 3, "the control needs batches the rotation changes"
    with pytest.raises(AssertionError, match="differ from the model on that block alone"):
        check(res, requests, want, want_pel)
    bad = SD.mismatches(res, want, want_pel)
    assert {b[2] for b in bad} == {SD.PEL, SD.F32} and {b[0] for b in bad} == set(SD.WIDTHS), "both kinds and every width are seen to be wrong"


def test_drive_reports_error_replies_and_stops_sending(oracle, load, sock_dir, monkeypatch):
    """A backend that fails: drive() returns the codes (it raises nothing), and every client stops at its next request."""
    _, requests, _, _ = load

    def failing(width, above, left):
        raise RuntimeError("no")

    monkeypatch.setenv("PNN_CACHE_MB", "0")
    sock = str(sock_dir / "pnn.sock")
    srv = service.serve_in_thread(sock, backend=failing, max_batch=8, window_us=0)
    res = SD.drive(sock, requests, 4)
    srv.stop(timeout=60)
    assert not res.hung and not res.answers
    assert 1 <= len(res.errors) <= 4 and all("-1" in e[4] for e in res.errors) and res.asked <= 4


def _lockstep_blocks(requests, w, n):
    above, left = requests[w]
    return [(above[i].copy(), None if left is None else left[i].copy()) for i in range(n)]


def test_a_refused_batch_is_reissued_and_the_error_stays_with_its_owner(oracle, load, sock_dir, monkeypatch):
    """include/pnn_service.h, "Errors stay with their owner", with a backend that refuses a call holding a non-finite input as
    pnn_predict_f32_pel does (PNN_E_ARG): the offender gets that code, the requests batched with it get the model's answers."""
    params, requests, want, want_pel = load
    right = model_backend(oracle, params)
    calls = []

    def backend(width, above, left):
        finite = bool(np.isfinite(above).all())
        calls.append((len(above), finite))
        return right(width, above, left) if finite else -1

    monkeypatch.setenv("PNN_SERVICE_WORKERS", "5")
    monkeypatch.setenv("PNN_CACHE_MB", "0")
    sock = str(sock_dir / "pnn.sock")
    srv = service.serve_in_thread(sock, backend=backend, max_batch=256, window_us=2000)
    blocks = _lockstep_blocks(requests, 8, 12)
    blocks[5][0][17] = np.nan
    kinds = [SD.PEL if k % 2 else SD.F32 for k in range(12)]
    got, hung = SD.drive_lockstep(sock, 8, blocks, kinds, rounds=6)
    stats = srv.stop(timeout=60)
    assert not hung
    assert any(n > 1 and not finite for n, finite in calls), "the offender must have travelled in a batch"
    assert got[5] == [-1] * 6
    for k in range(12):
        if k != 5:
            assert len(got[k]) == 6
            for g in got[k]:
                assert not isinstance(g, int), "client %d was answered %s for its neighbour's input" % (k, g)
                assert np.array_equal(g, (want_pel if kinds[k] == SD.PEL else want)[8][k]), k
    assert stats["requests"] == 72 and stats["backend_calls"] == len(calls)


def test_a_hip_error_is_replied_to_the_whole_batch_and_never_retried(sock_dir, monkeypatch):
    """PNN_E_HIP (-4) from the backend: every request of that batch gets it, and the batch is issued once."""
    calls = []

    def backend(width, above, left):
        calls.append(len(above))
        if (above[:, 0] == 54321.0).any():
            return -4
        return np.tile(np.round(above.sum(axis=1)).astype(np.int32)[:, None, None], (1, width, width))

    monkeypatch.setenv("PNN_CACHE_MB", "0")
    sock = str(sock_dir / "pnn.sock")
    srv = service.serve_in_thread(sock, backend=backend, max_batch=256, window_us=2000)
    blocks = [(np.full(80, float(k), np.float32), None) for k in range(8)]
    blocks[3][0][0] = 54321.0
    got, hung = SD.drive_lockstep(sock, 4, blocks, [SD.PEL] * 8, rounds=5)
    stats = srv.stop(timeout=60)
    assert not hung and got[3] == [-4] * 5
    answered = sum(len(g) for g in got)
    assert answered == 40 and stats["requests"] == 40
    assert stats["backend_calls"] == len(calls) and sum(calls) == 40, "no request was issued twice"
    shared = sum(1 for k in range(8) if k != 3 for g in got[k] if isinstance(g, int))
    assert shared > 0 and all(g == -4 for k in range(8) for g in got[k] if isinstance(g, int)), "the failed batch held more than the marked request"
    for k in range(8):
        if k != 3:
            for g in got[k]:
                assert isinstance(g, int) or np.array_equal(g, np.full((4, 4), 80 * k, np.int32))
