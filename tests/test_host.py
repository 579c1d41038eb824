"""CPU tests of the host side: the C ABI exports what include/pnn_hip.h declares, the host-only entry points
(context gather, descriptor builder, model-table parser) match the oracle / the reference's fixtures, and
the Python mirror keeps the reference's argument checks.  No compute call needs a GPU here."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from context_adaptive_neural_network_based_prediction_amd import _lib, weights as wts
from context_adaptive_neural_network_based_prediction_amd import prediction_neural_network as pn
from context_adaptive_neural_network_based_prediction_amd import sharding
from tests import util

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")


def test_abi_exports_every_declared_symbol():
    header = open(os.path.join(ROOT, "include", "pnn_hip.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    declared = set(re.findall(r"\b(pnn_[a-z0-9_]+)\s*\(", header))
    assert len(declared) >= 20
    L = _lib.lib()
    for name in sorted(declared):
        assert hasattr(L, name), "libpnn_hip.so does not export %s" % name
    assert declared == set(_lib.SIGNATURES), "ctypes binding and header disagree: %s" % (declared ^ set(_lib.SIGNATURES))
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH]).decode()
    exported = set(re.findall(r" T (pnn_[a-z0-9_]+)", out))
    assert declared <= exported


def test_device_code_has_no_packed_fp32_instructions(tmp_path):
    """gfx950 erratum found in round 1 (tools/pkfma_probe.hip, csrc/Makefile): a v_pk_fma_f32 whose destination pair is
    also its broadcast source pair can read a half that it has already overwritten while another wave on the SIMD issues
    MFMAs -- rare one-pixel errors whenever a second stream or context shares the chip.  The library is therefore built
    without packed-fp32 VALU code; this checks every code object embedded in the shipped .so."""
    llvm = "/opt/rocm/lib/llvm/bin"
    tools = [os.path.join(llvm, t) for t in ("llvm-objcopy", "clang-offload-bundler", "llvm-objdump")]
    if not all(os.path.exists(t) for t in tools):
        pytest.skip("ROCm LLVM binutils not installed")
    fat = str(tmp_path / "fat.bin")
    subprocess.run([tools[0], "--dump-section", ".hip_fatbin=" + fat, _lib.LIB_PATH, os.devnull], check=True)
    blob = open(fat, "rb").read()
    magic = b"__CLANG_OFFLOAD_BUNDLE__"
    starts = [m.start() for m in re.finditer(re.escape(magic), blob)]
    assert starts, "no offload bundle in .hip_fatbin"
    n_objects = n_mfma = 0
    kernels_seen = set()
    for i, a in enumerate(starts):
        piece = str(tmp_path / ("bundle%d.bin" % i))
        open(piece, "wb").write(blob[a:starts[i + 1] if i + 1 < len(starts) else len(blob)])
        co = str(tmp_path / ("dev%d.co" % i))
        subprocess.run([tools[1], "--unbundle", "--type=o", "--input=" + piece, "--targets=hipv4-amdgcn-amd-amdhsa--gfx950",
                        "--output=" + co], check=True)
        if not os.path.exists(co) or os.path.getsize(co) == 0:
            continue
        asm = subprocess.run([tools[2], "-d", co], check=True, capture_output=True, text=True).stdout
        n_objects += 1
        n_mfma += len(re.findall(r"\bv_mfma_", asm))
        bad = sorted(set(re.findall(r"\bv_pk_(?:fma|mul|add)_f32\b", asm)))
        assert not bad, "code object %d contains %s" % (i, bad)
        kernels_seen.update(re.findall(r"<_ZN3pnn\d+([a-z_0-9]+?)(?:I|E)", asm))
    assert n_objects >= 5 and n_mfma > 1000           # really looked at the kernels
    # every kernel family has device code in the shipped library: hipcc once emitted a host object WITHOUT its .hip_fatbin section,
    # with exit code 0 (an LDS-DMA builtin called straight from a lambda inside a __global__ template, pnn_convimg_sp.hip)
    for family in ("tapgemm_f32_kernel", "tapgemm_ring_kernel", "convimg_sp_kernel", "tapgemm_sp_kernel", "tapgemm_small_kernel", "tapgemm_f32_small_kernel",
                   "conv_cin1_kernel", "merger_mfma_kernel", "tconv_cout1_mfma_kernel", "fuse_reduce_kernel", "fc_out_f32_kernel", "block_cost_kernel"):
        assert any(k.startswith(family) for k in kernels_seen), "no device code for %s in %s" % (family, _lib.LIB_PATH)


def test_option_table_matches_the_header():
    """pnn_set_option's option table (kOptions, csrc/pnn_abi.cpp) and the option list in include/pnn_hip.h must not drift apart:
    every option name and environment variable of the table is documented there, and every one documented there is in the table."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = open(os.path.join(root, "context_adaptive_neural_network_based_prediction_amd", "csrc", "pnn_abi.cpp")).read()
    hdr = open(os.path.join(root, "include", "pnn_hip.h")).read()
    table = re.search(r"const OptionRow kOptions\[\] = \{(.*?)\n\};", src, re.S).group(1)
    rows = re.findall(r'\{"([a-z_0-9]+)",\s*(?:&pnn_ctx::\w+|nullptr),\s*(?:"(PNN_[A-Z0-9_]+)"|nullptr),', table)
    assert len(rows) == len(re.findall(r"^\s*\{", table, re.M)), "a table row the pattern does not read"
    names = {n for n, _ in rows}
    envs = {e for _, e in rows if e}
    assert len(names) == len(rows) and len(names) >= 30 and len(envs) >= 20, (sorted(names), sorted(envs))
    missing = sorted(n for n in names if '"%s"' % n not in hdr) + sorted(e for e in envs if not re.search(r"\b%s\b" % e, hdr))
    assert not missing, "options without documentation in pnn_hip.h: %s" % missing
    # ... and the other way round: the option list in front of pnn_set_option and the environment variables read at pnn_create*
    doc = hdr[hdr.index("/* Options (name, default, meaning)"):hdr.index("int pnn_set_option(")]
    env_doc = hdr[hdr.index("/* Environment variables read at pnn_create*"):hdr.index("Diagnostics:")]
    documented = set(re.findall(r'"([a-z_0-9]+)"', doc + env_doc))
    documented_env = set(re.findall(r"\bPNN_[A-Z0-9_]+\b", env_doc))
    assert documented_env and documented, "the option lists of pnn_hip.h moved"
    unknown = sorted(documented - names) + sorted(documented_env - envs)
    assert not unknown, "pnn_hip.h documents options the library does not have: %s" % unknown


def test_service_header_symbols_exported():
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pnn_service.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(pnn_(?:service|client)_[a-z0-9_]+)\s*\(", header))
    assert declared == set(_lib.SERVICE_SIGNATURES)
    L = _lib.lib()
    for name in declared:
        assert hasattr(L, name), "libpnn_hip.so does not export %s" % name


def test_batching_service_routes_and_coalesces(sock_dir):
    """include/pnn_service.h on the CPU with a stand-in backend (sum of the inputs per block): several client threads,
    mixed widths and both input kinds; every client gets ITS result, and concurrent requests are served in batches."""
    import threading
    from context_adaptive_neural_network_based_prediction_amd import service

    def backend(width, above, left):
        s = above.sum(axis=1) + (0 if left is None else left.sum(axis=1))
        ramp = np.arange(width * width, dtype=np.int64).reshape(1, width, width)
        return (np.round(s).astype(np.int64)[:, None, None] + ramp).astype(np.int32)

    sock = str(sock_dir / "pnn.sock")
    srv = service.serve_in_thread(sock, backend=backend, max_batch=8, window_us=3000)
    errors = []

    def client(k):
        try:
            c = service.Client(sock)
            rs = np.random.RandomState(k)
            for it in range(40):
                w = (4, 8, 16)[(k + it) % 3]
                if w <= 8:
                    a, l = rs.randint(-100, 100, 5 * w * w).astype(np.float32), None
                else:
                    a, l = rs.randint(-100, 100, 3 * w * w).astype(np.float32), rs.randint(-100, 100, 2 * w * w).astype(np.float32)
                got = c.predict_pel(w, a, l)
                want = backend(w, a[None], None if l is None else l[None])[0]
                if not np.array_equal(got, want):
                    errors.append((k, it))
            c.close()
        except Exception as e:                          # pragma: no cover
            errors.append((k, repr(e)))

    threads = [threading.Thread(target=client, args=(k,)) for k in range(6)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    stats = srv.stop()
    assert not errors, errors
    assert srv.rc == 0
    assert stats["requests"] == 240 and stats["clients"] == 6
    assert stats["backend_calls"] < stats["requests"] and 2 <= stats["largest_batch"] <= 8


def test_no_gpu_fails_loudly():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    ctx = ctypes.c_void_p()
    rc = _lib.lib().pnn_create_empty(ctypes.byref(ctx), ctypes.c_float(0.0), 0)
    assert rc != 0 and b"no CPU fallback" in _lib.lib().pnn_last_error(None)
    with pytest.raises(_lib.PnnError):
        pn.PredictionNeuralNetwork(1, 8, True, params=np.zeros(wts.param_count(8, True), np.float32))


def _host_extract(plane, x, y, w, flags, mean, n_avail=None):
    L = _lib.lib()
    plane = np.ascontiguousarray(plane, np.int32)
    flags = np.ascontiguousarray(flags, np.uint8)
    units = 2 * w // 4
    above = np.full((w, 3 * w), np.nan, np.float32)
    left = np.full((2 * w, w), np.nan, np.float32)
    origin = ctypes.cast(plane.ctypes.data + 4 * (y * plane.shape[1] + x), _lib.i32p)
    rc = L.pnn_extract_context(origin, above.ctypes.data_as(_lib.f32p), left.ctypes.data_as(_lib.f32p),
                               flags.ctypes.data_as(_lib.u8p), int(flags.sum()) if n_avail is None else n_avail, 4, 4,
                               units, units, w, w, plane.shape[1], ctypes.c_float(mean))
    return rc, above, left


def test_host_extract_context_matches_reference_goldens():
    g = np.load(os.path.join(GOLD, "gather_ref.npz"))
    for k in range(int(g["n_cases"])):
        w = int(g["c%d_w" % k])
        x, y = g["c%d_xy" % k]
        rc, a, l = _host_extract(g["c%d_plane" % k], int(x), int(y), w, g["c%d_flags" % k], float(g["c%d_mean" % k]))
        assert rc == 0
        assert np.array_equal(a, g["c%d_above" % k]) and np.array_equal(l, g["c%d_left" % k]), "case %d" % k


def test_host_extract_context_matches_oracle_random(oracle):
    for j in range(150):
        w = [4, 8, 16, 32, 64][j % 5]
        plane = util.make_plane(3 * w + 8, 3 * w + 16, seed=1000 + j)
        xs, ys, flags = util.make_tbs(plane.shape[0], plane.shape[1], w, 1, seed=j, partial_fraction=0.9, holes=j % 2 == 0)
        r0 = oracle.extract_context(plane, int(xs[0]), int(ys[0]), w, flags[0], util.MEAN)
        r1 = _host_extract(plane, int(xs[0]), int(ys[0]), w, flags[0], util.MEAN)
        assert r0[0] == r1[0] == 0 and np.array_equal(r0[1], r1[1]) and np.array_equal(r0[2], r1[2])


def test_host_extract_context_errors(capfd):
    plane = np.zeros((64, 64), np.int32)
    flags = np.ones(9, np.uint8)
    flags[4] = 0
    assert _host_extract(plane, 16, 16, 8, flags, 0.0)[0] == -1          # corner unit unavailable
    assert "above and on the left side" in capfd.readouterr().err
    assert _host_extract(plane, 16, 16, 8, np.ones(9, np.uint8), 0.0, n_avail=0)[0] == -1
    L = _lib.lib()
    assert L.pnn_extract_context(None, None, None, None, 1, 4, 4, 2, 2, 4, 4, 8, ctypes.c_float(0)) == -1


def test_make_tb_desc_semantics():
    L = _lib.lib()
    d = _lib.TbDev()
    units = 4                                                              # w = 8
    f = np.ones(9, np.uint8)
    assert L.pnn_make_tb_desc(ctypes.byref(d), 1234, 80, f.ctypes.data_as(_lib.u8p), 9, units, units) == 0
    assert (d.origin, d.stride, d.above_mask, d.left_units) == (1234, 80, 0xF, 4)
    f[0] = 0
    f[8] = 0                                                               # bottom-most below-left, right-most above-right
    assert L.pnn_make_tb_desc(ctypes.byref(d), 0, 80, f.ctypes.data_as(_lib.u8p), 7, units, units) == 0
    assert (d.above_mask, d.left_units) == (0x7, 3)
    f[:] = [1, 0, 1, 1, 1, 0, 1, 0, 1]                                     # holes: above masks per unit, left compacts
    assert L.pnn_make_tb_desc(ctypes.byref(d), 0, 80, f.ctypes.data_as(_lib.u8p), int(f.sum()), units, units) == 0
    assert (d.above_mask, d.left_units) == (0b1010, 3)
    f[4] = 0
    assert L.pnn_make_tb_desc(ctypes.byref(d), 0, 80, f.ctypes.data_as(_lib.u8p), int(f.sum()), units, units) == -1
    assert L.pnn_make_tb_desc(ctypes.byref(d), 0, 80, f.ctypes.data_as(_lib.u8p), 0, units, units) == -1


def _parse(path, cap=16):
    L = _lib.lib()
    w, p, c = (ctypes.c_int * cap)(), (ctypes.c_int * cap)(), (ctypes.c_int * cap)()
    paths = (ctypes.c_char_p * cap)()
    n = L.pnn_parse_model_table(path.encode(), w, p, c, paths, cap)
    return n, [(w[i], p[i], c[i], paths[i].decode()) for i in range(max(n, 0))]


def test_model_table_parser(tmp_path):
    # Same content as the reference's parser fixture hevc/hm_common/c++/pseudo_data/pseudo_file_strings_three_keys.txt:
    # blank lines, a whitespace-only line, leading blanks, ';' and ',' mixed, trailing blanks after the path.
    t = tmp_path / "table.txt"
    t.write_text("4,0,0,path_0\n\n\n 32;1;1;path_1\n8,1,2,path_2\n       \n64,0,2;path_3   \n32,0,1,path_4\n   ")
    n, rows = _parse(str(t))
    assert n == 5
    assert rows == [(4, 0, 0, "path_0"), (32, 1, 1, "path_1"), (8, 1, 2, "path_2"), (64, 0, 2, "path_3"), (32, 0, 1, "path_4")]
    # the tables HM ships (hevc/hm_common/paths_to_graphs_output/{single,pair}.txt) have this shape:
    t.write_text("".join("%d,%d,0,pnn/graphs_frozen/width_target_%d/x/graph_output.pbtxt\n" % (w, p, w)
                         for p in (0, 1) for w in (4, 8, 16, 32, 64)) + "\n\n")
    n, rows = _parse(str(t))
    assert n == 10 and rows[7] == (16, 1, 0, "pnn/graphs_frozen/width_target_16/x/graph_output.pbtxt")
    assert _parse(str(tmp_path / "missing.txt"))[0] < 0
    t.write_text("4,0\n")
    assert _parse(str(t))[0] < 0


def test_pnn_create_reports_missing_table():
    ctx = ctypes.c_void_p()
    L = _lib.lib()
    assert L.pnn_create(ctypes.byref(ctx), b"/nonexistent/table.txt", 0, ctypes.c_float(0.0), 0) != 0
    assert b"cannot be opened" in L.pnn_last_error(None)


def test_weight_tooling_roundtrip(tmp_path):
    for w, fc in ((4, True), (8, False)):
        flat = wts.init_params(w, fc, seed=5, bias_std=0.1)
        assert flat.size == wts.param_count(w, fc)
        p = str(tmp_path / "m.pnnw")
        wts.save_pnnw(p, flat, w, fc)
        back, ww, ffc = wts.load_pnnw(p)
        assert ww == w and ffc == fc and np.array_equal(back, flat)
        parts = wts.split_params(flat, w, fc)
        assert list(parts) == [n for n, _, _ in wts.tensor_specs(w, fc)]
    assert wts.output_node_name(8, True) == "fully_connected/node_output"
    assert wts.output_node_name(16, False) == "convolutional/merger/transpose_convolution_3/node_output"   # TComPrediction.cpp:599
    assert wts.output_node_name(32, False) == "convolutional/merger/transpose_convolution_4/node_output"   # TComPrediction.cpp:595
    with open(str(tmp_path / "bad.pnnw"), "wb") as f:
        f.write(b"nope" * 16)
    with pytest.raises(ValueError):
        wts.load_pnnw(str(tmp_path / "bad.pnnw"))


def test_tf_bundle_reader_on_reference_checkpoint():
    pre = "/root/reference/pnn/results/width_target_4/convolutional/single/luminance/1_0/masks_tr_random/model_800000.ckpt"
    if not os.path.exists(pre + ".index"):
        pytest.skip("reference checkpoints are only present in the build container")
    flat = wts.params_from_tf_bundle(pre, 4, False)
    gold, _, _ = wts.load_pnnw(os.path.join(GOLD, "conv4_single.pnnw"))
    assert np.array_equal(flat, gold)
    t = wts.read_tf_bundle(pre)
    assert int(t["learning_rate/global_step"]) == 800000 and "convolutional/merger/transpose_convolution_1/weights/Adam" in t


def test_batching_argument_checks():
    class Fake(object):
        is_fully_connected = True
        width_target = 4

        def predict(self, x):
            return np.zeros((x.shape[0], 4, 4, 1), np.float32)

    x = np.zeros((6, 80), np.float32)
    assert pn.predict_by_batch_via_pnn((x,), None, Fake(), 2).shape == (6, 4, 4, 1)
    with pytest.raises(ValueError):                       # batching.py:52-53 via tools.divide_ints_check_divisible
        pn.predict_by_batch_via_pnn((x,), None, Fake(), 4)
    with pytest.raises(ValueError):                       # batching.py:61-63: sqrt(cols / 5) is not whole
        pn.predict_by_batch_via_pnn((np.zeros((6, 81), np.float32),), None, Fake(), 2)
    with pytest.raises(TypeError):
        pn.divide_ints_check_divisible(6.0, 2)
    with pytest.raises(NotImplementedError):
        pn.PredictionNeuralNetwork(1, 8, True, tuple_coeffs=(1.0, 0.0))
    with pytest.raises(ValueError):
        pn.PredictionNeuralNetwork(1, 12, False)


def test_shard_bounds():
    for n, world in ((4096, 8), (1000, 3), (5, 8), (0, 2)):
        cover = []
        for r in range(world):
            b, e = sharding.shard_bounds(n, r, world)
            assert 0 <= b <= e <= n
            cover += list(range(b, e))
        assert cover == list(range(n))
        sizes = [sharding.shard_bounds(n, r, world)[1] - sharding.shard_bounds(n, r, world)[0] for r in range(world)]
        assert max(sizes) - min(sizes) <= 1
    with pytest.raises(ValueError):
        sharding.shard_bounds(10, 2, 2)


_WORKER = r'''
import os, sys, time
sys.path.insert(0, %(root)r)
import numpy as np, torch, torch.distributed as dist
from context_adaptive_neural_network_based_prediction_amd import sharding
from oracle import pnn_oracle as O
from tests import util
rank, local_rank, world = sharding.rank_env()
assert (rank, world) == (int(os.environ["RANK"]), 2) and local_rank == 0
assert sharding.init_ranks("gloo") is dist          # the same helper bench.py joins the job with ("nccl" there)
w, n = 4, 37                                   # ragged on purpose: 19 + 18
params = util.make_params(w, True, 1, out_gain=util.out_gain(w, True))
plane = util.make_plane(64, 96, seed=3)
xs, ys, flags = util.make_tbs(64, 96, w, n, seed=4)
b, e = sharding.shard_bounds(n, rank, world)
local = O.predict_tbs(params, w, True, plane, xs[b:e], ys[b:e], flags[b:e], util.MEAN)   # stands in for the GPU shard
full = sharding.gather_predictions(torch.from_numpy(local), n, dist).numpy()
want = O.predict_tbs(params, w, True, plane, xs, ys, flags, util.MEAN)
assert np.array_equal(full, want), "rank %%d: gathered shards differ from the unsharded result" %% rank
t = sharding.max_over_ranks(0.5 + rank, dist)
assert t == 0.5 + world - 1
# bench.py's timed region, driven here by a CPU step: exactly K steps between barriers, time = the slowest rank's
calls = []
def step():
    calls.append(1)
    time.sleep(0.02 * (rank + 1))               # rank 1 is twice as slow
k = 5
t = sharding.timed_steps(step, k, lambda: None, dist)
assert len(calls) == k
assert 0.02 * world * k <= t < 0.02 * world * k + 0.5, t
both = [None, None]
dist.all_gather_object(both, t)
assert both[0] == both[1], "ranks disagree on the job's time: %%r" %% (both,)
# the clock stops BEFORE the closing rendezvous: a rank that is late to it does not lengthen the region
t2 = sharding.timed_steps(lambda: None, 3, (lambda: time.sleep(0.3 * rank)) , dist)    # `sync` of rank 1 is slow; two of its three calls precede t0
assert t2 < 0.3 + 0.25, t2
# bench.py's rccl_ranks_seen: two ranks on one host, same local device 0 -> one distinct device in share mode, two otherwise
assert sharding.count_distinct_devices(dist, rank, share=False) == 2
assert sharding.count_distinct_devices(dist, rank, share=True) == 1
dist.barrier()
dist.destroy_process_group()
print("rank %%d ok" %% rank)
'''


def test_two_rank_sharding_gloo(tmp_path, oracle):
    """world_size-2 CPU run of the N > 1 path: contiguous shards, no data-path collective, results gathered in
    rank order equal the unsharded result; the step clock is the max over ranks."""
    script = tmp_path / "worker.py"
    script.write_text(_WORKER % {"root": ROOT})
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT="29533", WORLD_SIZE="2", OMP_NUM_THREADS="2")
    procs = [subprocess.Popen([sys.executable, str(script)], env=dict(env, RANK=str(r)), stdout=subprocess.PIPE,
                              stderr=subprocess.STDOUT) for r in range(2)]
    outs = [p.communicate(timeout=240)[0].decode() for p in procs]
    for r, (p, o) in enumerate(zip(procs, outs)):
        assert p.returncode == 0, "rank %d failed:\n%s" % (r, o)
        assert "rank %d ok" % r in o


def test_forced_one_rank_group_gloo(tmp_path):
    """bench.py --gpus 1 --force-dist: a process group of ONE rank, and every exchange of sharding.py -- barrier, max-over-ranks clock,
    device census, gather of the predictions -- goes through it instead of taking the single-process shortcut.  On the GPU box with
    "nccl" this is the only execution of the RCCL branch one device allows (tests/test_gpu_parity.py); here the same code over gloo."""
    script = tmp_path / "one_rank.py"
    script.write_text('''
import os, sys
sys.path.insert(0, %r)
import torch
import torch.distributed as dist
from context_adaptive_neural_network_based_prediction_amd import sharding
assert sharding.init_ranks("gloo") is None                      # no group without the flag ...
calls = {"all_reduce": 0, "all_gather": 0, "barrier": 0}
for name in calls:
    def wrap(name=name, fn=getattr(dist, name)):
        def f(*a, **k):
            calls[name] += 1
            return fn(*a, **k)
        return f
    setattr(dist, name, wrap())
d = sharding.init_ranks("gloo", force=True)                      # ... and one of ONE rank with it
assert d is dist and dist.get_world_size() == 1 and sharding.FORCE_COLLECTIVES
assert sharding.max_over_ranks(0.25, d) == 0.25 and calls["all_reduce"] == 1
probe = torch.arange(3 * 16, dtype=torch.int32).reshape(3, 4, 4)
assert torch.equal(sharding.gather_predictions(probe, 3, d), probe) and calls["all_gather"] == 1
n = []
t = sharding.timed_steps(lambda: n.append(1), 7, lambda: None, d)
assert len(n) == 7 and t >= 0 and calls["barrier"] == 1 and calls["all_reduce"] == 2
assert sharding.count_distinct_devices(d, 0) == 1
dist.destroy_process_group()
print("ok")
''' % ROOT)
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT="29547")
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, str(script)], env=env, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0 and "ok" in r.stdout, r.stdout + r.stderr


def test_tf_compat_headers_compile(tmp_path):
    """include/pnn_tf_compat.h + the shadow tree include/tf_compat/tensorflow/core/...: (1) the reference's own TF glue
    (integration_prediction_neural_network.cpp: create_tensors_*, load_graph(s)) compiles UNCHANGED against them when
    the reference checkout is present; (2) the call-site sample program compiles and links against libpnn_hip.so."""
    inc = ["-I" + os.path.join(ROOT, "include", "tf_compat"), "-I" + os.path.join(ROOT, "include")]
    ref = "/root/reference/hevc/hm_common/c++/source_common"
    if os.path.exists(os.path.join(ref, "integration_prediction_neural_network.cpp")):
        subprocess.check_call(["g++", "-std=c++11", "-fsyntax-only", "-Wall"] + inc + ["-I" + ref,
                              os.path.join(ref, "integration_prediction_neural_network.cpp")])
    exe = str(tmp_path / "hm_sample")
    libdir = os.path.dirname(_lib.LIB_PATH)
    subprocess.check_call(["g++", "-std=c++11", "-Wall"] + inc + [os.path.join(ROOT, "tests", "hm_callsite_sample.cpp"), "-o", exe,
                           "-L" + libdir, "-lpnn_hip", "-Wl,-rpath," + libdir])
    assert os.path.exists(exe)


def _pb_varint(n):
    out = bytearray()
    while True:
        b = n & 0x7F
        n >>= 7
        out.append(b | (0x80 if n else 0))
        if not n:
            return bytes(out)


def _pb_field(num, payload):                              # length-delimited field
    return _pb_varint((num << 3) | 2) + _pb_varint(len(payload)) + payload


def _pb_const_node(name, arr, use_float_val=False):
    shape = b"".join(_pb_field(2, _pb_varint((1 << 3) | 0) + _pb_varint(d)) for d in arr.shape)
    tensor = _pb_varint((1 << 3) | 0) + _pb_varint(1) + _pb_field(2, shape)
    tensor += _pb_field(5, arr.astype("<f4").tobytes()) if use_float_val else _pb_field(4, arr.astype("<f4").tobytes())
    attr = _pb_field(1, b"value") + _pb_field(2, _pb_field(8, tensor))
    return _pb_field(1, _pb_field(1, name.encode()) + _pb_field(2, b"Const") + _pb_field(5, attr))


def test_frozen_graphdef_reader(tmp_path):
    """A binary GraphDef with the layout freeze_graph produces (Const nodes named like the variables),
    hand-encoded here with a minimal protobuf writer: weights come back in the canonical order."""
    w, fc = 4, False
    flat = wts.init_params(w, fc, seed=9, bias_std=0.1)
    parts = wts.split_params(flat, w, fc)
    blob = _pb_field(1, _pb_field(1, b"node_portion_above") + _pb_field(2, b"Placeholder"))
    for i, (name, arr) in enumerate(parts.items()):
        blob += _pb_const_node(name, arr, use_float_val=(i % 5 == 4))
    blob += _pb_field(1, _pb_field(1, b"convolutional/merger/transpose_convolution_1/node_output") + _pb_field(2, b"BiasAdd"))
    path = str(tmp_path / "graph_output.pbtxt")
    with open(path, "wb") as f:
        f.write(blob)
    back = wts.params_from_frozen_graph(path, w, fc)
    assert np.array_equal(back, flat)
    out = str(tmp_path / "m.pnnw")
    wts.convert_model(path, out, w, fc)
    assert np.array_equal(wts.load_pnnw(out)[0], flat)
    with pytest.raises((KeyError, ValueError)):
        wts.params_from_frozen_graph(path, 8, False)       # a width-8 net does not match this file's tensors


def test_batching_service_survives_bad_clients(sock_dir):
    """One client that stops in the middle of a header, one that sends a malformed header and one that never reads its
    reply must not delay or break the others (the server is non-blocking with per-client buffers); a repeated request is
    answered from the client-side cache without reaching the server."""
    import socket
    import struct
    import time
    from context_adaptive_neural_network_based_prediction_amd import service

    def backend(width, above, left):
        if above[0, 0] == 12345.0:
            time.sleep(0.15)                                  # the request of the client that is killed meanwhile (below)
        return np.tile(np.round(above.sum(axis=1)).astype(np.int32)[:, None, None], (1, width, width))

    sock = str(sock_dir / "pnn.sock")
    srv = service.serve_in_thread(sock, backend=backend, max_batch=8, window_us=500)
    good = service.Client(sock)
    stalled = socket.socket(socket.AF_UNIX, socket.SOCK_STREAM)
    stalled.connect(sock)
    stalled.sendall(b"PNN2\x04\x00")                      # 6 of 20 header bytes, then silence
    junk = socket.socket(socket.AF_UNIX, socket.SOCK_STREAM)
    junk.connect(sock)
    junk.sendall(struct.pack("<IiIII", 0xdeadbeef, 4, 80, 0, 0))
    deaf = socket.socket(socket.AF_UNIX, socket.SOCK_STREAM)
    deaf.connect(sock)
    deaf.sendall(struct.pack("<IiIII", 0x324e4e50, 4, 80, 0, 0) + np.ones(80, np.float32).tobytes())   # valid; reply never read
    t0 = time.time()
    for i in range(50):
        a = np.full(80, float(i), np.float32)
        assert np.array_equal(good.predict_pel(4, a), np.full((4, 4), 80 * i, np.int32))
    assert time.time() - t0 < 5.0, "the good client was held up by the bad ones"
    assert junk.recv(16) == b""                            # malformed header: connection closed by the server
    # a client that DIES with a request in its shared-memory slot (round 6: requests travel through a slot per client, the socket is
    # the control channel): the worker that holds the request answers into memory nobody reads, the closing socket unlists the slot,
    # and the others are served on -- the same for a slot whose request is still only posted
    for rnd, delay in enumerate((0.05, 0.0)):
        victim = subprocess.Popen([sys.executable, "-c", "import sys, numpy as np\nsys.path.insert(0, %r)\n"
                                   "from context_adaptive_neural_network_based_prediction_amd import _lib, service\n_lib.SKIP_TORCH = True\n"
                                   "c = service.Client(%r)\nprint('up', flush=True)\na = np.zeros(80, np.float32); a[0] = 12345.0\nc.predict_pel(4, a)\n" % (ROOT, sock)],
                                  stdout=subprocess.PIPE, text=True)
        assert victim.stdout.readline().strip() == "up"
        time.sleep(delay)
        victim.kill()
        victim.wait()
        for i in range(5):
            a = np.full(80, 100.0 + 10 * rnd + i, np.float32)
            assert np.array_equal(good.predict_pel(4, a), np.full((4, 4), 80 * (100 + 10 * rnd + i), np.int32))
    hits, misses = ctypes.c_long(), ctypes.c_long()
    L = _lib.lib()
    again = good.predict_pel(4, np.full(80, 7.0, np.float32))
    assert np.array_equal(again, np.full((4, 4), 560, np.int32))
    L.pnn_client_cache_stats(good._c, ctypes.byref(hits), ctypes.byref(misses))
    assert hits.value == 1 and misses.value == 60
    good.close()
    stats = srv.stop()
    assert srv.rc == 0 and 61 <= stats["requests"] <= 63 and stats["clients"] == 6   # 60 + the deaf client's one (+ the victims' where the worker took them before they died)
    for s in (stalled, junk, deaf):
        s.close()


def test_arithmetic_tag_travels_through_the_service_and_the_session_checks_it(tmp_path, sock_dir, monkeypatch):
    """The arithmetic contract, enforced: the batching service reports the tag of what answers a width
    (pnn_client_arithmetic_tag: a flag in the request header, answered by the I/O thread), and the TensorFlow look-alike's
    Session::Create fails with a clean "arithmetic mismatch" when $PNN_EXPECT_TAG names another one -- instead of a decoder that
    drifts from its encoder.  No GPU: a stand-in backend behind the real server, the call-site sample program as the HM side."""
    from context_adaptive_neural_network_based_prediction_amd import service, weights as wts
    from tests import util

    def backend(width, above, left):
        s = above.sum(axis=1) + (left.sum(axis=1) if left is not None and left.size else 0.0)
        f32 = np.tile(s.astype(np.float32)[:, None, None], (1, width, width))
        return np.clip(np.round(f32), 0, 255).astype(np.int32), f32

    monkeypatch.setenv("PNN_SERVICE_TAG", "stand-in:f32:test order 7")
    sock = str(sock_dir / "pnn.sock")
    srv = service.serve_in_thread(sock, backend=backend, max_batch=8, window_us=0)
    cl = service.Client(sock)
    for w in (4, 8, 16, 32, 64):
        assert cl.arithmetic_tag(w) == "stand-in:f32:test order 7"
    a = np.arange(80, dtype=np.float32)
    assert np.array_equal(cl.predict_f32(4, a), np.full((4, 4), a.sum(), np.float32))       # a tag request leaves the connection usable
    assert cl.arithmetic_tag(4) == "stand-in:f32:test order 7"
    buf = ctypes.create_string_buffer(8)                                                        # a short buffer gets a truncated, terminated string
    assert _lib.lib().pnn_client_arithmetic_tag(cl._c, 4, buf, 8) == 0 and buf.value == b"stand-i"
    assert _lib.lib().pnn_client_arithmetic_tag(cl._c, 5, buf, 8) == -1                     # PNN_E_ARG
    cl.close()
    # the HM side: Session::Create behind the service, with and without the expectation
    wts.save_pnnw(str(tmp_path / "fc8.pnnw"), util.make_params(8, True, 41), 8, True)
    wts.save_pnnw(str(tmp_path / "conv16.pnnw"), util.make_params(16, False, 42), 16, False)
    inc = ["-I" + os.path.join(ROOT, "include", "tf_compat"), "-I" + os.path.join(ROOT, "include")]
    exe = str(tmp_path / "hm_sample")
    libdir = os.path.dirname(_lib.LIB_PATH)
    subprocess.check_call(["g++", "-std=c++11", "-Wall"] + inc + [os.path.join(ROOT, "tests", "hm_callsite_sample.cpp"), "-o", exe,
                           "-L" + libdir, "-lpnn_hip", "-Wl,-rpath," + libdir])
    argv = [exe, str(tmp_path / "fc8.pnnw"), "8", str(tmp_path / "conv16.pnnw"), "16"]
    env = dict(os.environ, PNN_SERVICE_SOCKET=sock, PNN_CACHE_MB="0")
    ok = subprocess.run(argv, env=dict(env, PNN_EXPECT_TAG="stand-in:f32:test order 7", PNN_PRINT_TAG="1"), capture_output=True, text=True, timeout=60)
    assert ok.returncode == 0, ok.stderr
    assert "arithmetic tag, width 8 (service): stand-in:f32:test order 7" in ok.stderr
    plain = subprocess.run(argv, env=env, capture_output=True, text=True, timeout=60)             # no expectation: nothing is asked, nothing fails
    assert plain.returncode == 0 and plain.stdout == ok.stdout
    bad = subprocess.run(argv, env=dict(env, PNN_EXPECT_TAG="pnn-order-6:f32:something else"), capture_output=True, text=True, timeout=60)
    assert bad.returncode == 1 and bad.stdout == ""
    assert "arithmetic mismatch for width 8" in bad.stderr and "stand-in:f32:test order 7" in bad.stderr and "something else" in bad.stderr
    stats = srv.stop()
    assert srv.rc == 0 and stats["requests"] == 1 + 2 * 2                                       # tag requests never reach the backend


def test_batching_service_many_clients_over_io_threads(sock_dir, monkeypatch):
    """The server's socket side runs on several I/O threads (a connection belongs to one of them for life; the workers hand a
    reply to the owner's queue): 48 clients on 4 I/O threads, 60 requests each over the five widths and both input shapes -- every
    reply must be the answer to ITS request, and clients that vanish in the middle must not disturb the rest."""
    import threading
    from context_adaptive_neural_network_based_prediction_amd import service

    def backend(width, above, left):
        s = above.sum(axis=1) + (left.sum(axis=1) if left is not None and left.size else 0.0)
        return np.tile(np.round(s).astype(np.int32)[:, None, None], (1, width, width))

    monkeypatch.setenv("PNN_SERVICE_IO_THREADS", "4")
    monkeypatch.setenv("PNN_CACHE_MB", "0")                  # every request reaches the server
    sock = str(sock_dir / "pnn.sock")
    srv = service.serve_in_thread(sock, backend=backend, max_batch=16, window_us=0)
    bad = []

    def client(k):
        rng = np.random.RandomState(k)
        c = service.Client(sock)
        try:
            for it in range(60):
                w = int(rng.choice([4, 8, 16, 32]))
                if (k + it) % 2:
                    a = rng.randint(0, 5, 5 * w * w).astype(np.float32)
                    got, want = c.predict_pel(w, a), int(a.sum())
                else:
                    a, l = rng.randint(0, 5, 3 * w * w).astype(np.float32), rng.randint(0, 5, 2 * w * w).astype(np.float32)
                    got, want = c.predict_pel(w, a, l), int(a.sum() + l.sum())
                if not np.array_equal(got, np.full((w, w), want, np.int32)):
                    bad.append((k, it))
                if k % 12 == 11 and it == 20:
                    return                                    # this client just goes away (its connection is closed below)
        finally:
            c.close()
    ts = [threading.Thread(target=client, args=(k,)) for k in range(48)]
    for t in ts:
        t.start()
    for t in ts:
        t.join(120)
    stats = srv.stop()
    assert not bad, bad[:5]
    assert srv.rc == 0 and stats["clients"] == 48 and stats["requests"] == 44 * 60 + 4 * 21


def test_host_code_under_sanitizers(sock_dir):
    """the host-only part of the library (context gather, descriptor builder, model-table parser,
    batching server + client incl. misbehaving clients) and the CPU oracle under AddressSanitizer + UBSan
    (`make -C csrc sanitize`, driver tests/sanitize_host.cpp).  Any report aborts the driver."""
    csrc = os.path.join(ROOT, "context_adaptive_neural_network_based_prediction_amd", "csrc")
    env = dict(os.environ, TMPDIR=str(sock_dir))
    r = subprocess.run(["make", "-C", csrc, "sanitize"], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "sanitize_host: ok" in r.stdout
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr


def test_service_under_thread_sanitizer(sock_dir):
    """`make -C csrc tsan`: the batching service -- server in its production thread layout (five width workers, four I/O
    threads) and client stub -- under ThreadSanitizer, driven by tests/tsan_service.cpp: 32 client threads against a stand-in backend
    with randomised latencies, with and without a batching window, clients that reconnect / vanish mid-request / die with a request in
    flight, tag requests, a server stopped under load.  Any report ends the run with exit code 66.  (3000 requests per client here,
    `make tsan` alone runs 10000: profiles/r06_tsan_service.txt.)  CPU build only."""
    csrc = os.path.join(ROOT, "context_adaptive_neural_network_based_prediction_amd", "csrc")
    env = dict(os.environ, TMPDIR=str(sock_dir))
    r = subprocess.run(["make", "-C", csrc, "tsan", "N=3000"], env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "tsan_service: ok" in r.stdout and "ThreadSanitizer" not in r.stdout + r.stderr


def test_model_table_parser_against_the_reference_parser(tmp_path):
    """pnn_parse_model_table (csrc/pnn_host.cpp) vs the REFERENCE's parse_file_strings_three_keys (tools.cpp:52-111, built into
    oracle/_ref/libref_tools.so by oracle/Makefile) on fuzzed tables: runs of ',' / ';' delimiters, blank and whitespace-only
    lines, padded fields, keys with trailing text, CRLF line ends, duplicate keys (later lines win), files with and without a
    final newline.  Where the reference throws (a line with fewer than four fields, a key that is not a number) this
    parser returns PNN_E_IO."""
    ref_path = os.path.join(ROOT, "oracle", "_ref", "libref_tools.so")
    if not os.path.exists(ref_path):
        pytest.skip("oracle/_ref/libref_tools.so not built (no /root/reference here)")
    R = ctypes.CDLL(ref_path)
    R.ref_parse_three_keys.restype = ctypes.c_int
    R.ref_parse_three_keys.argtypes = [ctypes.c_char_p, ctypes.c_char_p, ctypes.c_char_p, ctypes.c_int]
    L = _lib.lib()
    rng = np.random.RandomState(11)
    ws = [" ", "  ", "\t", ""]

    def pad(tok):
        return ws[rng.randint(len(ws))] + tok + ws[rng.randint(len(ws))]

    def good_line():
        w = str(rng.choice([4, 8, 16, 32, 64]))
        if rng.rand() < 0.15:
            w += "px"                                  # std::stoul stops at the first non-digit
        fields = [w, str(rng.randint(0, 3)), str(rng.randint(0, 3)), "dir %d/model_%d.pnnw" % (rng.randint(3), rng.randint(50))]
        seps = ["".join(rng.choice([",", ";"], rng.randint(1, 3))) for _ in range(3)]
        return pad(fields[0]) + seps[0] + pad(fields[1]) + seps[1] + pad(fields[2]) + seps[2] + pad(fields[3])

    n_ok = n_bad = 0
    for case in range(300):
        lines = []
        for _ in range(rng.randint(0, 12)):
            r = rng.rand()
            if r < 0.2:
                lines.append(ws[rng.randint(len(ws))] * rng.randint(0, 3))          # blank / whitespace-only
            elif r < 0.27 and case % 3 == 0:
                lines.append(rng.choice(["4,0,0", "x,0,0,p", "4,,0", "8;1"]))        # malformed
            else:
                lines.append(good_line())
        eol = "\r\n" if case % 5 == 0 else "\n"
        text = eol.join(lines) + (eol if case % 2 else "")
        path = str(tmp_path / ("t%d.txt" % case))
        with open(path, "w", newline="") as f:
            f.write(text)
        buf = ctypes.create_string_buffer(1 << 16)
        nref = R.ref_parse_three_keys(path.encode(), b",;", buf, len(buf))
        widths, pairs, chans = (ctypes.c_int * 64)(), (ctypes.c_int * 64)(), (ctypes.c_int * 64)()
        paths = (ctypes.c_char_p * 64)()
        n = L.pnn_parse_model_table(path.encode(), widths, pairs, chans, paths, 64)
        if nref == -2:                                  # the reference threw
            assert n == -2, (case, text, n)
            n_bad += 1
            continue
        assert nref >= 0 and n >= 0, (case, text, nref, n)
        want = {}
        for l in buf.value.decode().splitlines():
            w, p, c, v = l.split(" ", 3)
            want[(int(w), int(p), int(c))] = v
        got = {}
        for i in range(n):
            got[(widths[i], pairs[i], chans[i])] = paths[i].decode()               # later lines overwrite, as in std::map
        assert got == want, (case, text, got, want)
        n_ok += 1
    assert n_ok > 150 and n_bad > 10
    assert R.ref_parse_three_keys(str(tmp_path / "absent.txt").encode(), b",;", buf, len(buf)) == -1
    assert L.pnn_parse_model_table(str(tmp_path / "absent.txt").encode(), widths, pairs, chans, paths, 64) == -2


def test_bench_self_launch_without_a_gpu():
    """`python bench.py --gpus 2` run plainly (no launcher, WORLD_SIZE unset) must start its own ranks as a child process and
    relay their fate: here, without a GPU, a clear refusal before any rank is started (the node exposes 0 GPUs), and in share
    mode the children's own "no HIP device" error with a non-zero code -- never a traceback about a missing launcher."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "PNN_BENCH_SHARE_GPU"):
        env.pop(k, None)
    import torch
    if torch.cuda.device_count() >= 2:
        pytest.skip("a multi-GPU node: the real thing runs instead")
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1", "--scaling", "strong"], env=env, capture_output=True,
                       text=True, timeout=300, cwd=root)
    # the preflight of the self-launching parent: ONE JSON line in the result line's shape, value null, the reason spelled out
    import json
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert r.returncode != 0 and len(lines) == 1, r.stdout[-2000:] + r.stderr[-2000:]
    d = json.loads(lines[0])
    assert d["value"] is None and d["n_gpus"] == 2 and d["scaling"] == "strong" and d["metric"] == "pnn_intra_pred_blocks_per_s"
    assert "this node exposes" in d["error"] and d["devices_visible"] == torch.cuda.device_count()
    if torch.cuda.device_count() == 0:
        env["PNN_BENCH_SHARE_GPU"] = "1"
        r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1"], env=env, capture_output=True,
                           text=True, timeout=300, cwd=root)
        assert r.returncode != 0 and "no HIP device visible" in r.stderr, r.stderr[-2000:]
        assert not [l for l in r.stdout.splitlines() if l.startswith("{")]


def _canned_measurement(name, precision, lsb=0):
    import bench
    w, fc, batch, _ = bench.WORKLOADS[name]
    return {"value": 1.6234567e7, "unit": "blocks/s", "ms_per_step": 0.25234567, "dtype": bench.DTYPE_LONG[precision], "precision": precision, "steps": 20,
            "workload": name, "batch_per_gpu": batch, "launches_per_step": 14, "max_abs_lsb_vs_oracle": lsb,
            "repeats": {"n": 5, "ms_per_step_all": [0.25234567] * 5}, "pred_psnr": {"gpu_db": 11.123456, "oracle_db": 11.123456, "delta_db": 1.234e-7},
            "roofline": {"bound": "mfma", "kernel": "tapgemm_ring_kernel (same split-product MFMAs; 4 MFMA + 4 loader waves, LDS-DMA ring; incl. the fused output layer)",
                         "achieved": 118.7654321, "peak": 157.3, "unit": "TFLOP/s", "frac": 0.7550123456, "traffic": 59355500.61482544,
                         "traffic_source": "this run: rocprofv3 --pmc FETCH_SIZE x2 + WRITE_SIZE", "flops_per_launch": 8912345678.9, "avg_launch_us": 75.0123456,
                         "launches_timed": 150, "held_sclk_mhz": 1904.123456, "frac_at_held_clock": 0.4512345678,
                         "whole_pass": {"tflops": 107.123456, "frac_of_peak": 0.681234567, "issued_frac_of_peak": 0.612345678, "issued_over_algorithmic": 0.8312345}}}


def test_bench_line_fits_the_driver_tail_buffer():
    """The ONE JSON line bench.py prints must stay below 4 KB whatever the run measured (round 3's 24 KB line lost its head --
    value, roofline, cpu_baseline -- in the driver's 8 KB tail buffer): build_line on canned results of every sub-measurement,
    with the longest strings and full-precision floats the real run can produce."""
    import json
    import bench
    main = _canned_measurement("fc8", 0, lsb=1)
    fast = _canned_measurement("fc8", 1)
    per_width = {n: {"f32": _canned_measurement(n, 0), "split": _canned_measurement(n, 1)} for n in bench.PER_WIDTH}
    cpu = {"value": 12345.678901, "unit": "blocks/s", "cores": 64, "host_cores": 256, "kind": "port", "value_leg": "torch_cpu_batched",
           "batch1_value": 234.5678901, "batch1_leg": "torch_cpu_batch1", "batch1_cores": 8, "sample": "x" * 600, "legs": {"bulk": "y" * 5000}}
    natural = {w: {"contexts": 2500, "oracle_db": 24.9501234567, "f32_db": 24.9501234567, "split_db": 24.9498765432, "f32_max_abs_lsb_vs_oracle": 1} for w in ("4", "8")}
    single = {n: {"us": 123.456789, "us_p10": 120.123456, "us_p90": 130.987654, "calls": 300, "blocks_per_s": 8100.123456, "param_bytes": 82610180,
                  "param_gbps": 669.123456, "frac_of_hbm": 0.0836404, "launches": 11, "entry_point": "pnn_predict_conv"} for n in bench.PER_WIDTH}
    line = bench.build_line(main, 8, 20, 5, bench.WORKLOADS["fc8"][3], fast, per_width, cpu, dict(cpu), "bench_detail.json",
                            {"plumbing_check": "PNN_BENCH_SHARE_GPU=1: all ranks on ONE device"}, {"backend": "nccl", "world_size": 8, "devices": 8}, natural, single)
    assert len(line) < bench.LINE_LIMIT and "\n" not in line, len(line)
    d = json.loads(line)
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype", "data", "config",
              "roofline", "cpu_baseline", "fast_arithmetic", "per_width", "rccl_ranks_seen", "natural_pred_psnr_db", "single_block"):
        assert k in d, k
    # the reference's call shape in the driver-run line: one block per host call, beside the CPU's batch-1 leg
    assert sorted(d["single_block"]) == ["conv16", "fc8"]
    for r in d["single_block"].values():
        assert {"us", "blocks_per_s", "param_gbps", "frac_of_hbm", "gpu_over_cpu_batch1"} <= set(r) and r["gpu_over_cpu_batch1"] > 1
    assert all("single_block_us" in row for row in d["per_width"].values())
    assert d["dtype"] == "f32" and d["n_gpus"] == 8 and d["config"]["workload"].startswith("configs[1]") and "model" not in d["config"]
    for k in ("bound", "kernel", "achieved", "peak", "unit", "frac", "traffic", "flops_per_launch", "avg_launch_us"):
        assert k in d["roofline"], k
    assert abs(d["roofline"]["frac"] - d["roofline"]["achieved"] / d["roofline"]["peak"]) < 2e-3
    for k in ("value", "unit", "cores", "kind", "sample"):
        assert k in d["cpu_baseline"], k
    assert sorted(d["per_width"]) == ["16", "32", "4", "64", "8"]
    for row in d["per_width"].values():
        assert row["arch"] in ("fc", "conv") and {"value", "frac", "lsb"} <= set(row["f32"]) and {"value", "frac", "lsb"} <= set(row["split"])
    # the minimal line (N > 1 ranks: no extras) carries the contract keys too
    d2 = json.loads(bench.build_line(main, 2, 20, 5, "w", rccl_ranks_seen={"backend": "nccl", "world_size": 2, "devices": 2}))
    assert d2["cpu_baseline"] is None and d2["rccl_ranks_seen"]["devices"] == 2 and d2["value"] == d["value"]


def test_bench_plain_line_says_what_it_measured():
    """A plain run (no --full) measures one region of K steps and nothing else: the line keeps the contract keys, and the figures it
    did not take -- roofline, oracle check, CPU baseline, extras -- are null or absent."""
    import json
    import bench
    main = {"value": 1.76789e7, "ms_per_step": 0.231688, "precision": 0, "batch_per_gpu": 4096, "scaling": "weak", "global_batch": 4096,
            "repeats": {"n": 1, "ms_per_step_all": [0.231688]}, "roofline": None}
    d = json.loads(bench.build_line(main, 1, 500, 5, bench.WORKLOADS["fc8"][3]))
    assert d["metric"] == "pnn_intra_pred_blocks_per_s" and d["unit"] == "blocks/s" and d["higher_is_better"] is True and d["dtype"] == "f32"
    assert d["value"] == 1.76789e7 and d["ms_per_step"] == 0.231688 and d["steps"] == 500 and d["warmup"] == 5
    assert d["config"]["timing"] == "one region of K steps"
    assert d["roofline"] is None and d["cpu_baseline"] is None and d["max_abs_lsb_vs_oracle"] is None and d["pred_psnr_delta_db"] is None
    assert not {"fast_arithmetic", "per_width", "single_block", "natural_pred_psnr_db", "detail_file"} & set(d)


def test_bench_dump_outputs(tmp_path, monkeypatch):
    """--dump-outputs: the last step's Pel blocks as float32 pred_pel.npy, exact; above the cap (shared by the ranks) a sample of
    blocks drawn with a fixed seed, its indices beside it -- the same sample every run, within the cap in all."""
    import types
    import torch
    import bench
    pel = np.random.RandomState(3).randint(0, 256, (4096, 8, 8)).astype(np.int32)
    wl = types.SimpleNamespace(d_dst=torch.from_numpy(pel))
    bench.dump_outputs(wl, str(tmp_path / "all"), 0)
    got = np.load(str(tmp_path / "all" / "pred_pel.npy"))
    assert got.dtype == np.float32 and np.array_equal(got, pel) and sorted(os.listdir(str(tmp_path / "all"))) == ["pred_pel.npy"]
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 200000)
    for run in ("a", "b"):
        for rank in (0, 1):
            bench.dump_outputs(wl, str(tmp_path / run), rank, world=2)
    total = 0
    for tag in ("", "_rank1"):
        got = np.load(str(tmp_path / "a" / ("pred_pel%s.npy" % tag)))
        idx = np.load(str(tmp_path / "a" / ("pred_pel%s_index.npy" % tag)))
        assert got.dtype == np.float32 and idx.dtype == np.float64 and 0 < got.shape[0] < pel.shape[0]
        assert np.array_equal(got, pel[idx.astype(np.int64)]) and np.all(np.diff(idx) > 0)
        assert np.array_equal(idx, np.load(str(tmp_path / "b" / ("pred_pel%s_index.npy" % tag))))
        total += got.nbytes + idx.nbytes
    assert total <= 200000


def test_gpu_placement_helpers(tmp_path):
    """sharding's sysfs readers on a fake KFD / DRM tree: GPUs in KFD order, HIP_VISIBLE_DEVICES remapping, cpulist parsing,
    NUMA binding to the cores that are both local to the GPU and allowed to this process."""
    from context_adaptive_neural_network_based_prediction_amd import sharding
    assert sharding.parse_cpulist("0-3,8,10-11\n") == [0, 1, 2, 3, 8, 10, 11]
    kfd, drm = tmp_path / "kfd", tmp_path / "drm"
    allowed = sorted(os.sched_getaffinity(0))
    for i, (simd, minor) in enumerate([(0, 0), (1024, 129), (1024, 128)]):
        (kfd / str(i)).mkdir(parents=True)
        (kfd / str(i) / "properties").write_text("cpu_cores_count 64\nsimd_count %d\ndrm_render_minor %d\n" % (simd, minor))
    for minor, cpus in ((128, "%d" % allowed[0]), (129, "%d-%d" % (allowed[0], allowed[-1]))):
        (drm / ("renderD%d" % minor) / "device").mkdir(parents=True)
        (drm / ("renderD%d" % minor) / "device" / "local_cpulist").write_text(cpus + "\n")
    assert sharding.gpu_render_minors(str(kfd)) == [129, 128]
    assert sharding.visible_device_index(1, {"HIP_VISIBLE_DEVICES": "3,1"}) == 1 and sharding.visible_device_index(1, {}) == 1
    assert sharding.gpu_sysfs_dir(1, str(kfd), str(drm)).endswith("renderD128/device")
    assert sharding.gpu_sysfs_dir(5, str(kfd), str(drm)) is None
    before = os.sched_getaffinity(0)
    try:
        if len(allowed) > 1:
            assert sharding.bind_to_gpu_numa(1, str(kfd), str(drm)) == [allowed[0]]
            assert os.sched_getaffinity(0) == {allowed[0]}
            os.sched_setaffinity(0, before)
        assert sharding.bind_to_gpu_numa(0, str(kfd), str(drm)) is None     # the whole machine is "local": nothing to bind
    finally:
        os.sched_setaffinity(0, before)
    assert sharding.GpuClockSampler(7).summary() is None or True


def _stagger_rank(rank, world, port, out):
    import time
    import torch.distributed as dist
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import bench
    from context_adaptive_neural_network_based_prediction_amd import sharding
    d = sharding.init_ranks("gloo")
    stamps = []

    def fn():
        stamps.append(time.time())
        time.sleep(0.2)
        stamps.append(time.time())
    bench.stagger(d, fn)
    out.put((rank, stamps))
    d.destroy_process_group()


def test_staggered_first_calls_two_ranks_gloo():
    """bench.py's first (autotuning) call of a workload runs one rank after the other (bench.stagger): with two gloo ranks the
    two 0.2 s sections must not overlap, rank 0 first."""
    import multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    ps = [ctx.Process(target=_stagger_rank, args=(r, 2, 29733, q)) for r in range(2)]
    for p in ps:
        p.start()
    res = dict(q.get(timeout=120) for _ in ps)
    for p in ps:
        p.join(60)
        assert p.exitcode == 0
    assert res[0][1] <= res[1][0] + 1e-3, res


def test_strong_scaling_shards_and_encodes_in_flight():
    """bench.py --scaling strong: ONE batch split over the ranks by shard_bounds (every rank at least one block); campaigns size their
    encoder pool by the CPUs the job may really use (the cgroup quota), oversubscribed -- encoders behind the service wait, they do not
    compute -- with one CPU set aside per service (configs[4] on 8 GPUs under the boxes' 16-CPU quota: 64 of the 100 encodes)."""
    from context_adaptive_neural_network_based_prediction_amd import sharding
    for total, world in ((4096, 8), (1024, 8), (4096, 3), (7, 7)):
        got = [sharding.strong_shard(total, r, world) for r in range(world)]
        assert sum(c for _, c in got) == total and all(c >= 1 for _, c in got)
        assert all(got[r + 1][0] == got[r][0] + got[r][1] for r in range(world - 1)) and got[0][0] == 0
        assert max(c for _, c in got) - min(c for _, c in got) <= 1
    with pytest.raises(ValueError):
        sharding.strong_shard(3, 7, 8)
    assert sharding.encodes_in_flight(100, 8, budget=16) == 64
    assert sharding.encodes_in_flight(24, 1, budget=16) == 24 and sharding.encodes_in_flight(100, 1, budget=16) == 100
    assert sharding.encodes_in_flight(100, 8, budget=256) == 100
    assert sharding.encodes_in_flight(100, 8, budget=4) == 8          # never fewer than one encode per service
    assert sharding.encodes_in_flight(3, 8, budget=16) == 8


def test_bench_strong_scaling_two_ranks_gloo(tmp_path):
    """The bookkeeping of --scaling strong through two real ranks (gloo on the CPU, a stand-in step): each rank takes its shard of ONE
    batch, regions are at least 200 steps, the job's value is global_batch x steps / the slowest rank's time -- not N x the shard."""
    import multiprocessing as mp
    import bench  # noqa: F401  (the module under test must import without a GPU)
    port = 29650 + os.getpid() % 200

    def rank_main(rank, q):
        os.environ.update({"RANK": str(rank), "LOCAL_RANK": str(rank), "WORLD_SIZE": "2", "MASTER_ADDR": "127.0.0.1", "MASTER_PORT": str(port)})
        import time
        from context_adaptive_neural_network_based_prediction_amd import sharding
        dist = sharding.init_ranks("gloo")
        b0, mine = sharding.strong_shard(4097, rank, 2)
        steps = max(20, 200)
        t = sharding.timed_steps(lambda: time.sleep(1e-5 * (1 + rank)), steps, lambda: None, dist)
        q.put((rank, b0, mine, steps, t))
        dist.destroy_process_group()
    ctx = mp.get_context("fork")
    q = ctx.Queue()
    ps = [ctx.Process(target=rank_main, args=(r, q)) for r in range(2)]
    for p in ps:
        p.start()
    res = sorted(q.get(timeout=120) for _ in ps)
    for p in ps:
        p.join(60)
        assert p.exitcode == 0
    assert [(r[1], r[2]) for r in res] == [(0, 2049), (2049, 2048)]
    assert res[0][3] == res[1][3] == 200 and res[0][4] == pytest.approx(res[1][4])      # both ranks report the slowest rank's time
    value = 4097 * 200 / res[0][4]
    assert value < 4097 * 200 / (200 * 2e-5)                            # bounded by the SLOW rank's 20 us steps


def test_cpu_budget_reads_the_cgroup_quota(tmp_path, monkeypatch):
    """bench.cpu_budget(): the CPU legs may use what the cgroup grants, not what os.cpu_count() shows (the GPU boxes: 256 cores, quota 16)."""
    import builtins
    import bench
    n = bench.cpu_budget()
    assert 1 <= n <= (os.cpu_count() or 1)
    real_open = builtins.open

    def fake(quota_text):
        def _open(path, *a, **k):
            if str(path) == "/sys/fs/cgroup/cpu.max":
                f = tmp_path / "cpu.max"
                f.write_text(quota_text)
                return real_open(f, *a, **k)
            return real_open(path, *a, **k)
        return _open
    monkeypatch.setattr(os, "sched_getaffinity", lambda pid: set(range(256)), raising=False)
    monkeypatch.setattr(builtins, "open", fake("1600000 100000\n"))
    assert bench.cpu_budget() == 16
    monkeypatch.setattr(builtins, "open", fake("max 100000\n"))
    assert bench.cpu_budget() == 256
    monkeypatch.setattr(builtins, "open", fake("50000 100000\n"))
    assert bench.cpu_budget() == 1
