"""The production batching service on the GPU -- pnn_service_run_table: five contexts, four adopted queue streams, "wait_sleep" and
the deep weight ring, slots and doorbells behind four I/O threads, batches of 1 to max_batch -- against the bit-exact CPU model of the
f32 summation order (oracle/pnn_order.c) at ZERO tolerance: every answer of every client, Pel or float, is the model on that block
alone followed by the HM epilogue.  The load and the clients are tests/service_driver.py (proved on the CPU by
tests/test_service_driver.py, negative control included; nothing here is made to fail on purpose).  The split-f16 mode, which has no
bit-level model, is compared with direct single-block calls on plain contexts (bit for bit) and with float64.

Every case runs one server thread and at most 12 client threads in this process; every join has a limit, and a case stops sending at
its first wrong answer.  Each case prints its server statistics; with $PNN_SERVICE_DEBUG the server adds calls and requests per width.

Wall time (pytest's own figures): 12.00 s for this file; with 150 instead of 120 blocks for each FC width 12.08 s, beside 12.07 s for
tests/test_f32_contract.py on the same MI355X box.  About 0.45 s of every case is the start and stop of its five-context server; the first choice of
600 / 600 / 200 / 48 / 16 blocks took 14.7 s against 11.6 s, so the request counts were cut (tests/service_driver.py, COUNTS), not the cases.
"""
import ctypes
import os

import numpy as np
import pytest

from context_adaptive_neural_network_based_prediction_amd import _lib, service, weights as wts
from tests import service_driver as SD
from tests import test_f32_contract as F32C
from tests import torch_formulation as TF
from tests import util

pytestmark = pytest.mark.gpu

PNN_E_ARG = -1                                        # include/pnn_hip.h
SEEDS = {4: 804, 8: 808, 16: 816, 32: 832, 64: 864}
N_CLIENTS = 12
N_REQUESTS = sum(SD.COUNTS.values())


def _unflatten(w, above, left):
    """(above [n][w][3w], left [n][2w][w]) of a width's requests, as the order model's helpers of test_f32_contract.py take them."""
    if left is not None:
        return above, left
    n = above.shape[0]
    return above[:, :3 * w * w].reshape(n, w, 3 * w), above[:, 3 * w * w:].reshape(n, 2 * w, w)


class Load(object):
    pass


@pytest.fixture(scope="module")
def load(oracle, tmp_path_factory):
    """The table, the requests of the issue's counts and the order model's answers: the model computes block after block, each from
    its own inputs alone, so row i is the model on block i alone (tests/test_service_driver.py checks that)."""
    ld = Load()
    ld.dir = tmp_path_factory.mktemp("service")
    ld.table, ld.params = SD.make_table(ld.dir, SEEDS, conv_gain=3.0)     # both clamps of the epilogue at every width
    ld.requests = SD.make_requests(seed=870)
    ld.want, ld.want_pel = {}, {}
    for w in SD.WIDTHS:
        a, l = _unflatten(w, *ld.requests[w])
        ld.want[w] = F32C._model(oracle, ld.params[w], w, SD.is_fc(w), a, l)
        ld.want_pel[w] = oracle.epilogue(ld.want[w], util.MEAN)
        assert ld.want_pel[w].min() == 0 and ld.want_pel[w].max() == 255, "the inputs must exercise both clamps"
    return ld


@pytest.fixture(autouse=True)
def environment(monkeypatch):
    """What every case starts from: exact f32, no client cache (every request reaches a worker), the production layout."""
    for name in ("PNN_SERVICE_QUEUES", "PNN_SERVICE_SHM", "PNN_SERVICE_IO_THREADS", "PNN_SERVICE_WORKERS", "PNN_SERVICE_GROUPS",
                 "PNN_SERVICE_REPLICAS", "PNN_SERVICE_PRIORITIES", "PNN_WAIT_SLEEP", "PNN_F32_SMALL_DEEP"):
        monkeypatch.delenv(name, raising=False)
    monkeypatch.setenv("PNN_PRECISION", "0")
    monkeypatch.setenv("PNN_CACHE_MB", "0")


def _serve(sock_dir, table, **kw):
    sock = str(sock_dir / "pnn.sock")
    srv = service.serve_in_thread(sock, table=table, **kw)
    assert SD.wait_listening(srv, sock), "the service did not start: rc %s, %s" % (srv.rc, (_lib.lib().pnn_last_error(None) or b"").decode())
    return srv, sock


def _stop(srv, what):
    stats = srv.stop(timeout=60)
    assert srv.rc == 0, srv.rc
    print("service case %-28s requests %5d, backend calls %5d (%.2f requests per call), largest batch %3d, clients %2d"
          % (what + ":", stats["requests"], stats["backend_calls"], stats["requests"] / max(1, stats["backend_calls"]),
             stats["largest_batch"], stats["clients"]))
    return stats


def _wrong(ld):
    return lambda w, i, kind, got: not np.array_equal(got, (ld.want_pel if kind == SD.PEL else ld.want)[w][i])


def _verify(res, ld, oracle, what, asks=1):
    """Nobody hung, no error reply, every block answered `asks` times, every answer the model's -- a float mismatch is reported with
    the ladder of test_f32_contract.py (which single departure from the order reproduces the GPU's bits)."""
    assert not res.hung, "%s: client hung: %s" % (what, res.hung)
    assert not res.errors, "%s: %s" % (what, res.errors[:5])
    bad = SD.mismatches(res, ld.want, ld.want_pel)
    if bad:
        w, i, kind, ask = bad[0]
        got = res.answers[(w, i, kind)][ask]
        head = "%s: %d answers differ from the model, first: width %d, block %d, %s, ask %d" % (what, len(bad), w, i, kind, ask)
        if kind == SD.F32:
            a, l = _unflatten(w, *ld.requests[w])
            F32C._same_bits(got[None], ld.want[w][i:i + 1], head, oracle, (ld.params[w], w, SD.is_fc(w), a[i:i + 1], l[i:i + 1]))
        d = np.abs(got.astype(np.int64) - ld.want_pel[w][i])
        raise AssertionError("%s: %d of %d Pel values differ, max |delta| %d" % (head, int((d != 0).sum()), d.size, d.max()))
    assert res.asked == asks * N_REQUESTS and sum(len(v) for v in res.answers.values()) == asks * N_REQUESTS, what
    assert {k[:2] for k in res.answers} == {(w, i) for w in SD.WIDTHS for i in range(SD.COUNTS[w])}, what
    assert {(k[0], k[2]) for k in res.answers} == {(w, kind) for w in SD.WIDTHS for kind in (SD.PEL, SD.F32)}, "%s: both kinds at every width" % what


def test_five_widths_at_once_default_layout(load, oracle, sock_dir):
    srv, sock = _serve(sock_dir, load.table, max_batch=256, window_us=0)
    res = SD.drive(sock, load.requests, N_CLIENTS, with_tags=True, stop_on=_wrong(load))
    stats = _stop(srv, "default layout")
    _verify(res, load, oracle, "default layout")
    assert stats["requests"] == N_REQUESTS and stats["clients"] == N_CLIENTS
    assert res.tags == {k: {w: oracle.order_tag() for w in SD.WIDTHS} for k in range(N_CLIENTS)}


def test_a_window_makes_batches(load, oracle, sock_dir):
    srv, sock = _serve(sock_dir, load.table, max_batch=256, window_us=2000)
    res = SD.drive(sock, load.requests, N_CLIENTS, seed=2, stop_on=_wrong(load))
    stats = _stop(srv, "window 2000 us")
    _verify(res, load, oracle, "window 2000 us")
    assert stats["requests"] == N_REQUESTS
    assert stats["largest_batch"] >= 2 and stats["backend_calls"] < stats["requests"]


@pytest.mark.parametrize("w", [32, 64])
def test_the_big_widths_travel_in_common_batches(load, oracle, sock_dir, w):
    """In the shuffled load a 32x32 or 64x64 request seldom meets another one inside a window; here 12 clients send one each at the
    same moment, three times, so these widths are seen in batches of 2 and more (the server sees nothing else: largest_batch is theirs)."""
    srv, sock = _serve(sock_dir, load.table, max_batch=256, window_us=2000)
    blocks = [SD.block(load.requests, w, i) for i in range(N_CLIENTS)]
    kinds = [SD.F32 if k % 2 else SD.PEL for k in range(N_CLIENTS)]
    got, hung = SD.drive_lockstep(sock, w, blocks, kinds, rounds=3)
    stats = _stop(srv, "width %d in lockstep" % w)
    assert not hung, hung
    for k in range(N_CLIENTS):
        assert len(got[k]) == 3
        for g in got[k]:
            assert not isinstance(g, int), "client %d: error %s" % (k, g)
            if kinds[k] == SD.F32:
                a, l = load.requests[w]
                F32C._same_bits(g[None], load.want[w][k:k + 1], "width %d, block %d" % (w, k), oracle, (load.params[w], w, False, a[k:k + 1], l[k:k + 1]))
            else:
                assert np.array_equal(g, load.want_pel[w][k]), "width %d, block %d (Pel)" % (w, k)
    assert stats["requests"] == 3 * N_CLIENTS and stats["largest_batch"] >= 2 and stats["backend_calls"] < stats["requests"]


def test_the_max_batch_cut(load, oracle, sock_dir):
    """max_batch = 3 behind 12 clients and a window: the "leave the rest queued" branches of take()."""
    srv, sock = _serve(sock_dir, load.table, max_batch=3, window_us=2000)
    res = SD.drive(sock, load.requests, N_CLIENTS, seed=3, stop_on=_wrong(load))
    stats = _stop(srv, "max_batch 3")
    _verify(res, load, oracle, "max_batch 3")
    assert stats["requests"] == N_REQUESTS and stats["largest_batch"] == 3


@pytest.mark.parametrize("mixed", [False, True], ids=["socket", "half-socket-half-slots"])
def test_transports(load, oracle, sock_dir, mixed):
    env = [{"PNN_SERVICE_SHM": "0" if (k < N_CLIENTS // 2 or not mixed) else "1"} for k in range(N_CLIENTS)]
    srv, sock = _serve(sock_dir, load.table, max_batch=256, window_us=0)
    res = SD.drive(sock, load.requests, N_CLIENTS, env=env, seed=4, stop_on=_wrong(load))
    what = "half socket, half slots" if mixed else "socket protocol"
    stats = _stop(srv, what)
    _verify(res, load, oracle, what)
    assert stats["requests"] == N_REQUESTS and stats["clients"] == N_CLIENTS


def test_fallback_layout(load, oracle, sock_dir, monkeypatch):
    """$PNN_SERVICE_QUEUES=0: every context on the stream it created, one worker thread per width."""
    monkeypatch.setenv("PNN_SERVICE_QUEUES", "0")
    srv, sock = _serve(sock_dir, load.table, max_batch=256, window_us=0)
    res = SD.drive(sock, load.requests, N_CLIENTS, seed=5, stop_on=_wrong(load))
    stats = _stop(srv, "PNN_SERVICE_QUEUES=0")
    _verify(res, load, oracle, "PNN_SERVICE_QUEUES=0")
    assert stats["requests"] == N_REQUESTS


def test_back_to_back_loads_on_one_server(load, oracle, sock_dir):
    """Three loads without a restart: arrival counters, "wait_sleep" state and staging buffers from call to call."""
    srv, sock = _serve(sock_dir, load.table, max_batch=256, window_us=0)
    runs = []
    for rep in range(3):
        runs.append(SD.drive(sock, load.requests, N_CLIENTS, seed=10 + rep, stop_on=_wrong(load)))
        if runs[-1].hung or runs[-1].errors or SD.mismatches(runs[-1], load.want, load.want_pel):
            break
    stats = _stop(srv, "three loads back to back")
    for rep, res in enumerate(runs):
        _verify(res, load, oracle, "load %d of 3" % (rep + 1))
    assert len(runs) == 3 and stats["requests"] == 3 * N_REQUESTS and stats["clients"] == 3 * N_CLIENTS


def test_client_cache(load, oracle, sock_dir, monkeypatch):
    """$PNN_CACHE_MB at its default.  The cache is kept per (width, reply kind) -- a Pel reply cannot answer a float request -- so a
    repeat "for the other result kind" alone can never hit.  Every block is therefore asked four times in a row: kind A (first ask),
    the other kind (a first ask too: it must reach the server and must not be answered with A's bytes), then A and the other kind
    again (the repeats).  Hits = the repeats, server requests = the first asks, every answer exact."""
    monkeypatch.delenv("PNN_CACHE_MB")
    srv, sock = _serve(sock_dir, load.table, max_batch=256, window_us=0)
    res = SD.drive(sock, load.requests, N_CLIENTS, seed=6, asks=4, stop_on=_wrong(load))
    stats = _stop(srv, "client cache")
    _verify(res, load, oracle, "client cache", asks=4)
    assert all(len(v) == 2 for v in res.answers.values())
    assert sum(h for h, _ in res.cache.values()) == 2 * N_REQUESTS and sum(m for _, m in res.cache.values()) == 2 * N_REQUESTS
    for k, (h, m) in res.cache.items():
        assert h == m == 2 * sum(len(range(k, SD.COUNTS[w], N_CLIENTS)) for w in SD.WIDTHS), k
    assert stats["requests"] == 2 * N_REQUESTS


def test_a_request_of_the_wrong_shape_is_refused_and_the_connection_lives(load, oracle, sock_dir, monkeypatch):
    """Host-side checks only: a conv-shaped request to the FC width 8 and an FC-shaped one to the conv width 16, from a client on
    the slots and from one on the socket protocol."""
    srv, sock = _serve(sock_dir, load.table, max_batch=256, window_us=0)
    for shm in ("1", "0"):
        monkeypatch.setenv("PNN_SERVICE_SHM", shm)
        _refused_and_alive(load, service.Client(sock))
    stats = _stop(srv, "wrong shapes")
    assert stats["requests"] == 8 and stats["clients"] == 2, "a refused request never reaches a worker's batch"


def _refused_and_alive(load, c):
    L = _lib.lib()
    out = np.empty((16, 16), np.float32)
    a8, l8 = np.zeros(3 * 64, np.float32), np.zeros(2 * 64, np.float32)
    a16 = np.zeros(5 * 256, np.float32)
    for rep in range(2):
        assert L.pnn_client_predict_f32(c._c, 8, a8.ctypes.data_as(_lib.f32p), l8.ctypes.data_as(_lib.f32p), out.ctypes.data_as(_lib.f32p)) == PNN_E_ARG
        assert np.array_equal(c.predict_f32(8, *SD.block(load.requests, 8, rep)), load.want[8][rep])
        assert L.pnn_client_predict_f32(c._c, 16, a16.ctypes.data_as(_lib.f32p), None, out.ctypes.data_as(_lib.f32p)) == PNN_E_ARG
        assert np.array_equal(c.predict_pel(16, *SD.block(load.requests, 16, rep)), load.want_pel[16][rep])
    c.close()


def test_errors_stay_with_their_owner(load, oracle, sock_dir):
    """One client sends a width-8 context that holds a NaN, then one that holds an Inf, while 11 others send finite ones at the same
    moment behind a 2 ms window.  pnn_predict_f32_pel refuses a call with a non-finite input on the host (nothing reaches a kernel);
    the offender gets the code a direct call gives, every other client its exact prediction (include/pnn_service.h: a refused batch is
    re-issued in halves).  Before that rule the worker replied the batch's one code to all: the neighbours got PNN_E_ARG too."""
    import context_adaptive_neural_network_based_prediction_amd as P
    w, offender, rounds = 8, 5, 4
    net = P.PredictionNeuralNetwork(1, w, True, path_to_model=str(load.dir / "w8.pnnw"))
    srv, sock = _serve(sock_dir, load.table, max_batch=256, window_us=2000)
    kinds = [SD.PEL if k % 2 else SD.F32 for k in range(N_CLIENTS)]
    results = []
    for poison in (np.nan, np.inf):
        blocks = [tuple(None if x is None else x.copy() for x in SD.block(load.requests, w, i)) for i in range(N_CLIENTS)]
        blocks[offender][0][17] = poison
        out = np.empty((w, w), np.float32)
        direct = _lib.lib().pnn_predict_f32_pel(net.ctx, w, blocks[offender][0].ctypes.data_as(_lib.f32p), None, 1, out.ctypes.data_as(_lib.f32p), None)
        assert direct == PNN_E_ARG, direct
        got, hung = SD.drive_lockstep(sock, w, blocks, kinds, rounds)
        results.append((poison, direct, got, hung))
        if hung:
            break
    stats = _stop(srv, "NaN / Inf batch-mates")
    net.close()
    for poison, direct, got, hung in results:
        assert not hung, hung
        assert got[offender] == [direct] * rounds, "the offender (%s) got %s" % (poison, got[offender])
        shared = [(k, g) for k in range(N_CLIENTS) if k != offender for g in got[k] if isinstance(g, int)]
        assert not shared, "%d requests of other clients were answered with their batch-mate's refusal (%s), e.g. client %d: %d" % (
            len(shared), poison, shared[0][0], shared[0][1])
        for k in range(N_CLIENTS):
            if k != offender:
                assert len(got[k]) == rounds
                for g in got[k]:
                    assert np.array_equal(g, (load.want_pel if kinds[k] == SD.PEL else load.want)[w][k]), "client %d beside %s" % (k, poison)
    assert len(results) == 2 and stats["requests"] == 2 * rounds * N_CLIENTS and stats["largest_batch"] >= 2


def _direct_split(P, path, w, requests):
    """Single-block calls on a plain context (pnn_create_empty + pnn_load_model_file under $PNN_PRECISION=1): float and Pel per block."""
    net = P.PredictionNeuralNetwork(1, w, SD.is_fc(w), path_to_model=path)
    above, left = requests
    f32 = np.empty((len(above), w, w), np.float32)
    pel = np.empty((len(above), w, w), np.int32)
    for i in range(len(above)):
        ins = (above[i:i + 1],) if left is None else (above[i:i + 1], left[i:i + 1])
        f32[i] = net.predict(*ins)[0, ..., 0]
        pel[i] = net.predict_pel(*ins)[0]
    tag = net.arithmetic_tag()
    net.close()
    return f32, pel, tag


def test_split_mode_service_is_the_direct_call(load, oracle, sock_dir, tmp_path, monkeypatch):
    """$PNN_PRECISION=1 for the server: every answer = the direct single-block call on a plain context created the same way, bit for
    bit ("a block gets the same prediction whatever batch it travels in"); floats within FLOAT_ATOL of float64 and Pel by the
    tie-aware rule of test_f32_contract.py; the tag is not the f32 order's.  A table of its own: util.out_gain as it is, the gain
    test_split_mode_against_float64 holds FLOAT_ATOL at."""
    import context_adaptive_neural_network_based_prediction_amd as P
    monkeypatch.setenv("PNN_PRECISION", "1")
    table, params = SD.make_table(tmp_path, SEEDS)
    direct = Load()
    direct.requests, direct.params, direct.want, direct.want_pel = load.requests, params, {}, {}
    tags = set()
    for w in SD.WIDTHS:
        direct.want[w], direct.want_pel[w], tag = _direct_split(P, str(tmp_path / ("w%d.pnnw" % w)), w, load.requests[w])
        tags.add(tag)
        a, l = _unflatten(w, *load.requests[w])
        p64 = TF.fc_forward(params[w], w, util.flatten_fc(a, l), np.float64) if SD.is_fc(w) else TF.conv_forward(params[w], w, a, l, np.float64)
        np.testing.assert_allclose(direct.want[w], p64.reshape(direct.want[w].shape), rtol=0, atol=F32C.FLOAT_ATOL, err_msg="width %d, direct" % w)
        F32C._check_pel_tie_aware(direct.want_pel[w], p64.reshape(direct.want[w].shape), "width %d, direct" % w)
    assert len(tags) == 1 and tags != {oracle.order_tag()}
    srv, sock = _serve(sock_dir, table, max_batch=256, window_us=2000)
    res = SD.drive(sock, load.requests, N_CLIENTS, seed=7, with_tags=True, stop_on=_wrong(direct))
    stats = _stop(srv, "split-f16, window 2000 us")
    assert not res.hung and not res.errors, (res.hung, res.errors[:5])
    bad = SD.mismatches(res, direct.want, direct.want_pel)
    assert not bad, "%d answers differ from the direct single-block call, first (width, block, kind, ask): %s" % (len(bad), bad[:5])
    assert res.asked == N_REQUESTS and len(res.answers) == N_REQUESTS       # (equal to the direct calls, so inside the float64 bounds checked above)
    assert stats["requests"] == N_REQUESTS and stats["largest_batch"] >= 2
    assert res.tags == {k: {w: next(iter(tags)) for w in SD.WIDTHS} for k in range(N_CLIENTS)}
    with pytest.raises(ValueError):
        oracle.require_order_tag(res.tags[0][8])


@pytest.mark.parametrize("is_fc,w,n", [(True, 8, 9), (False, 16, 7)])
def test_split_mode_range_fallback_behind_the_service(load, oracle, sock_dir, tmp_path, monkeypatch, is_fc, w, n):
    """test_split_mode_range_fallback_is_the_f32_order behind the server: one client's block leaves the f16 range and must be the f32
    order model's; every block batched with it must be its direct split-mode answer."""
    import context_adaptive_neural_network_based_prediction_amd as P
    monkeypatch.setenv("PNN_PRECISION", "1")
    flat = util.make_params(w, is_fc, 91, out_gain=util.out_gain(w, is_fc)).copy()
    specs = wts.tensor_specs(w, is_fc)
    offs = np.concatenate([[0], np.cumsum([int(np.prod(sh)) for _, sh, _ in specs])])
    gain = 300.0 if is_fc else 1000.0
    flat[offs[0]:offs[2]] *= gain
    flat[offs[-3]:offs[-2]] /= gain
    wts.save_pnnw(str(tmp_path / ("w%d.pnnw" % w)), flat, w, is_fc)        # in place of the module's model of this width
    table = wts.write_model_table(str(tmp_path / "table.txt"), [(v, 0, 0, str((tmp_path if v == w else load.dir) / ("w%d.pnnw" % v))) for v in SD.WIDTHS])
    above, left = util.make_contexts(w, n, 92, masked_fraction=0.0)
    bad = n // 2
    above[bad] *= 40.0
    left[bad] *= 40.0
    want_bad = F32C._model(oracle, flat, w, is_fc, above[bad:bad + 1], left[bad:bad + 1])
    requests = (util.flatten_fc(above, left), None) if is_fc else (above, left)
    d_f32, d_pel, _ = _direct_split(P, str(tmp_path / ("w%d.pnnw" % w)), w, requests)
    F32C._same_bits(d_f32[bad:bad + 1], want_bad, "the overflowing block, direct call", oracle, (flat, w, is_fc, above[bad:bad + 1], left[bad:bad + 1]))
    srv, sock = _serve(sock_dir, table, max_batch=256, window_us=2000)
    blocks = [SD.block({w: requests}, w, i) for i in range(n)]
    kinds = [SD.F32 if k == bad or k % 2 else SD.PEL for k in range(n)]
    got, hung = SD.drive_lockstep(sock, w, blocks, kinds, rounds=3)
    stats = _stop(srv, "range fallback, width %d" % w)
    assert not hung, hung
    for k in range(n):
        assert len(got[k]) == 3
        for g in got[k]:
            assert not isinstance(g, int), "client %d: error %s" % (k, g)
            if k == bad:
                F32C._same_bits(g[None], want_bad, "the overflowing block behind the service", oracle, (flat, w, is_fc, above[bad:bad + 1], left[bad:bad + 1]))
            else:
                assert np.array_equal(g, (d_f32 if kinds[k] == SD.F32 else d_pel)[k]), "block %d beside the overflowing one" % k
    assert stats["requests"] == 3 * n and stats["largest_batch"] >= 2
