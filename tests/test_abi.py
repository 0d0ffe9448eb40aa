"""CPU: the C-ABI library builds, loads, and exports every symbol include/vaecap.h declares
(no compute calls without a GPU)."""
import ctypes
import os

import pytest

from vae_captioning_amd import abi


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()
    return abi.load()


def test_every_declared_symbol_is_exported(built):
    protos = abi.parse_header()
    assert len(protos) >= 45
    cdll = ctypes.CDLL(abi.LIB_PATH)
    missing = [n for n in protos if not hasattr(cdll, n)]
    assert not missing, missing


def test_every_prototype_maps_to_ctypes(built):
    for name, (ret, args) in abi.parse_header().items():
        assert ret in abi._CTYPES, (name, ret)
        for t, a in args:
            assert t in abi._CTYPES, (name, t, a)
        getattr(built, name)  # binds argtypes


def test_version_and_error_paths(built):
    assert built.vc_abi_version() == 4
    assert built.vc_sumsq_blocks() > 0
    assert built.vc_gemm_workspace_bytes(1280, 256, 15000) > 0
    assert built.vc_gemm_workspace_bytes(25600, 10000, 512) == 0
    # argument validation happens before any device work, so it is testable without a GPU
    with pytest.raises(abi.VaecapError) as e:
        built.vc_gemm_f32(None, 0, 0, 4, 4, 4, None, 4, None, 4, None, 4, None, 0, None, 0)
    assert "null operand" in str(e.value)
    with pytest.raises(abi.VaecapError):
        built.vc_lstm_step_fwd_f32(None, 8, 12, 0, 16, 16, 16, 16, 16, 16, 16)  # H % 32 != 0


def test_missing_library_fails_loudly(tmp_path):
    with pytest.raises(abi.VaecapError):
        abi.load(str(tmp_path / "nope.so"))


def test_no_device_is_an_error_not_a_fallback(built):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(abi.VaecapError):
        built.vc_device_check(0)


def test_product_code_never_touches_the_oracle_or_the_reference():
    """oracle/ is test infrastructure: only tests/, __graft_entry__.smoke() and bench.py's cpu_baseline leg may use it,
    and nothing that runs on the GPU box may read /root/reference."""
    import ast
    import glob
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    product = glob.glob(os.path.join(root, "vae_captioning_amd", "**", "*.py"), recursive=True) + \
        [os.path.join(root, f) for f in ("main.py", "gen_caption.py", "preprocess.py")]
    assert len(product) > 20
    for path in product:
        src = open(path).read()
        assert "/root/reference" not in src, path
        for node in ast.walk(ast.parse(src)):
            names = []
            if isinstance(node, ast.Import):
                names = [a.name for a in node.names]
            elif isinstance(node, ast.ImportFrom):
                names = [node.module or ""]
            assert not any(n == "oracle" or n.startswith("oracle.") for n in names), path
    for path in (os.path.join(root, "bench.py"), os.path.join(root, "__graft_entry__.py")):
        src = open(path).read()
        assert "/root/reference" not in src.replace('os.path.isdir("/root/reference")', ""), path
    bench = open(os.path.join(root, "bench.py")).read()
    # bench.py: the oracle appears only inside cpu_baseline()
    tree = ast.parse(bench)
    for node in tree.body:
        uses = any(isinstance(n, (ast.Import, ast.ImportFrom)) and "oracle" in ast.dump(n) for n in ast.walk(node))
        if uses:
            assert isinstance(node, ast.FunctionDef) and "cpu_baseline" in node.name, getattr(node, "name", node)


def test_bench_executed_ratio_of_the_winograd_kernels():
    """bench.py prices the Winograd kernels' executed MFMA work as a fraction of the algorithmic (direct-convolution) FLOPs.  Forward /
    data gradient: F(4x4,3x3) = 36 / 144 per layer and pass on every layer behind conv1_1 (csrc/conv_wino4.hip: blocks of
    16 x 16 pixels -- exact at 224 / 112; linear blocks of sixteen consecutive tiles at 56 / 28: every slot real; one block per image with
    (14 / 16)^2 = 49 / 64 of the slots real at 14; the library's own preference rule, which bench.py asks, takes all of them since round 4);
    weight gradient F(3x3,2x2) = 16 / 36 over plan_wino_wgrad's
    block coverage; conv1_1 stays direct.  Hand-worked for the VGG16 shapes at 224 x 224; the F(2x2,3x3)-only figure is kept beside it."""
    import bench
    r, r2 = bench.wino_executed_ratio(64), bench.wino_executed_ratio(64, wino4=False)
    # per layer: (forward / data-gradient multiplications per direct multiplication, weight-gradient block coverage)
    fd = {224: 0.25, 112: 0.25, 56: 0.25, 28: 0.25, 14: 0.25 / (49.0 / 64.0)}   # (56 / 28: linear tiles fill every slot; 14: 3.5 tiles per side)
    fd2 = {224: 16.0 / 36.0, 112: 16.0 / 36.0, 56: 16.0 / 36.0, 28: (16.0 / 36.0) / 0.875, 14: (16.0 / 36.0) / (49.0 / 64.0)}
    effw = {224: 1.0, 112: 1.0, 56: 1.0, 28: 1.0, 14: 0.875}
    layers = [(224, 3, 64), (224, 64, 64), (112, 64, 128), (112, 128, 128), (56, 128, 256), (56, 256, 256), (56, 256, 256),
              (28, 256, 512), (28, 512, 512), (28, 512, 512), (14, 512, 512), (14, 512, 512), (14, 512, 512)]
    alg = ex = ex2 = 0.0
    for H, ci, co in layers:
        fl = H * H * 9.0 * ci * co
        if ci == 3:
            alg += 2 * fl
            ex += 2 * fl
            ex2 += 2 * fl
        else:
            alg += 3 * fl
            ex += 2 * fl * fd[H] + fl * (16.0 / 36.0) / effw[H]
            ex2 += 2 * fl * fd2[H] + fl * (16.0 / 36.0) / effw[H]
    assert abs(r - ex / alg) < 1e-9 and abs(r2 - ex2 / alg) < 1e-9
    assert 0.31 < r < 0.34 and 0.46 < r2 < 0.49
    # split-bf16 mode: the weight gradients leave the f32 family (csrc/conv_wgrad_bx.hip prices them on the bf16 pipe) -- forward / data
    # gradient alone: 0.25 everywhere but the 14 x 14 layers, conv1_1's forward direct
    r3 = bench.wino_executed_ratio(64, with_wgrad=False)
    alg3 = sum((1 if ci == 3 else 2) * H * H * 9.0 * ci * co for H, ci, co in layers)
    ex3 = sum((1.0 if ci == 3 else 2 * fd[H]) * H * H * 9.0 * ci * co for H, ci, co in layers)
    assert abs(r3 - ex3 / alg3) < 1e-9 and 0.25 < r3 < 0.27


def test_plans_of_the_split_bf16_convolution_kernels(built):
    """host-side plan functions of csrc/conv_wgrad_bx.hip (no device needed): which shapes it takes and what its
    workspace is -- [K splits][9][Cin][Cout] raw sums + two rows of dy sums per split, channel tiles x splits = one
    workgroup per CU (256), blocks of eight stacked rows x sixteen columns"""
    lib = built
    for (B, H, ci, co) in [(64, 224, 64, 64), (64, 112, 128, 128), (64, 56, 256, 256), (32, 28, 512, 512), (64, 14, 512, 512), (1, 1, 64, 64)]:
        assert lib.vc_conv3x3_bx_wgrad_supported(B, H, H, ci, co) == 1
        tiles = (ci // 64) * (co // 64)
        nblocks = -(-H // 16) * -(-(B * (H + 1) - 1) // 8)
        ns = min(-(-256 // tiles), nblocks)
        cps = -(-nblocks // ns)
        nsplit = -(-nblocks // cps)
        assert lib.vc_conv3x3_bx_wgrad_workspace_bytes(B, H, H, ci, co) == (nsplit * 9 * ci * co + 2 * nsplit * co) * 4
        assert tiles * nsplit <= 256 or nblocks < 256
    assert lib.vc_conv3x3_bx_wgrad_supported(8, 8, 8, 32, 64) == 0 and lib.vc_conv3x3_bx_wgrad_supported(8, 8, 8, 64, 32) == 0
    assert lib.vc_conv3x3_bx_wgrad_supported(8, 0, 8, 64, 64) == 0 and lib.vc_conv3x3_bx_wgrad_workspace_bytes(8, 8, 8, 32, 64) == 0


def test_bench_algorithmic_bytes_of_the_convolution_calls():
    """roofline.traffic_over_algorithmic's denominator (bench.conv_algorithmic_bytes, formula in DESIGN.md section 6), hand-worked per image:
    every call reads its input and writes its output once; forwards add the pooled copy behind the five pools, data gradients the ReLU
    source (bits: 1/32 of the tensor -- since round 4 also conv1_2's, whose bits conv1_1's forward leaves; none behind a pool), all calls their 3x3
    weights."""
    import bench
    layers = [(224, 3, 64, 0), (224, 64, 64, 1), (112, 64, 128, 0), (112, 128, 128, 1), (56, 128, 256, 0), (56, 256, 256, 0), (56, 256, 256, 1),
              (28, 256, 512, 0), (28, 512, 512, 0), (28, 512, 512, 1), (14, 512, 512, 0), (14, 512, 512, 0), (14, 512, 512, 1)]
    B = 64
    acts = weights = 0.0
    for i, (H, ci, co, pooled) in enumerate(layers):
        px = B * H * H
        cin = 4 if ci == 3 else ci
        fwd = px * cin + px * co + (px // 4) * co * pooled
        wg = px * cin + px * co
        dg = 0.0
        if i > 0:
            behind_pool = layers[i - 1][3]
            mask = 0.0 if behind_pool else px * ci / 32.0
            dg = px * co + px * ci + mask
        acts += 4.0 * (fwd + wg + dg)
        weights += 4.0 * (9 * ci * co + co) * (3 if i > 0 else 2)
    got = bench.conv_algorithmic_bytes(B)
    assert abs(got - (acts + weights)) < 1e-3 * got
    assert 16.7e9 < got < 17.7e9   # ~17.2 GB per 64-image step = 269 MB per image


def test_bench_without_a_launcher_starts_its_own_ranks(monkeypatch):
    """`python bench.py --gpus 4 ...` with no WORLD_SIZE in the environment (the shape of the driver's scaling command if it does not wrap
    it in torchrun): bench.self_launch re-runs the same arguments under torch.distributed.run with one process per GPU, rendezvous on
    127.0.0.1 at a free port, and exits with the launcher's code.  (The two-rank run itself: tests/test_gpu_cli.py.)"""
    import subprocess
    import sys
    import bench
    seen = {}

    def fake_call(cmd, env=None):
        seen["cmd"], seen["env"] = cmd, env
        return 7
    monkeypatch.setattr(subprocess, "call", fake_call)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "4", "--steps", "3", "--warmup", "1", "--workload", "cfg2"])
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    with pytest.raises(SystemExit) as e:
        bench.main()
    assert e.value.code == 7
    cmd = seen["cmd"]
    assert cmd[0] == sys.executable and cmd[1:3] == ["-m", "torch.distributed.run"]
    assert cmd[cmd.index("--nproc-per-node") + 1] == "4" and cmd[cmd.index("--master-addr") + 1] == "127.0.0.1"
    assert 1024 < int(cmd[cmd.index("--master-port") + 1]) < 65536
    i = cmd.index(os.path.abspath(bench.__file__))
    assert cmd[i + 1:] == ["--gpus", "4", "--steps", "3", "--warmup", "1", "--workload", "cfg2"]
    assert "OMP_NUM_THREADS" in seen["env"]
    # under a launcher (WORLD_SIZE set) bench.py does not launch again; a world size that disagrees with --gpus is an error message
    monkeypatch.setenv("WORLD_SIZE", "2")
    seen.clear()
    with pytest.raises(SystemExit) as e:
        bench.main()
    assert not seen and "--gpus 4 but WORLD_SIZE=2" in str(e.value.code)


def test_bench_dump_outputs_sample_is_fixed_by_the_name():
    """bench.py --dump-outputs: an array up to DUMP_SAMPLE elements is written whole; above that, the same DUMP_SAMPLE elements (sorted
    indices from a generator seeded by the variable's name alone) whether the array is a host array or a tensor, so that two builds'
    dumps line up element for element."""
    import numpy as np
    import torch
    import bench
    small = np.arange(12, dtype=np.float32).reshape(3, 4)
    np.testing.assert_array_equal(bench._dump_sample("a/b", small), small.reshape(-1))
    big = np.arange(3 * (bench.DUMP_SAMPLE + 7), dtype=np.float32).reshape(-1, 3)   # distinct values (exact in float32)
    s1 = bench._dump_sample("cnn/fc1/weights", big)
    assert s1.dtype == np.float32 and s1.shape == (bench.DUMP_SAMPLE,)
    np.testing.assert_array_equal(s1, bench._dump_sample("cnn/fc1/weights", big.copy()))
    np.testing.assert_array_equal(s1, bench._dump_sample("cnn/fc1/weights", torch.from_numpy(big)))
    assert not np.array_equal(s1, bench._dump_sample("cnn/fc2/weights", big))
    assert len(np.unique(s1)) == bench.DUMP_SAMPLE and (np.diff(s1) > 0).all()   # distinct elements in array order
    assert bench._dump_name("decoder/rnn_logits/kernel") == "decoder__rnn_logits__kernel"


def test_bench_dump_outputs_of_beam_search(tmp_path):
    """cfg5's dump: per image the kept beams in the order beam_search returns them, token ids padded with -1, scores NaN where an
    image kept fewer beams than the beam width."""
    import numpy as np
    import bench
    res = [[([1, 5, 6, 2], -1.5), ([1, 7, 2], -2.0)], [([1, 9, 9, 9, 2], -0.25)]]
    bench.dump_beams(str(tmp_path), res, 3)
    ids, sc = np.load(tmp_path / "beam_ids.npy"), np.load(tmp_path / "beam_scores.npy")
    assert ids.dtype == np.float32 and ids.shape == (2, 3, 5) and sc.dtype == np.float64 and sc.shape == (2, 3)
    np.testing.assert_array_equal(ids[0, 0], [1, 5, 6, 2, -1])
    np.testing.assert_array_equal(ids[0, 1], [1, 7, 2, -1, -1])
    np.testing.assert_array_equal(ids[0, 2], [-1] * 5)
    np.testing.assert_array_equal(ids[1, 0], [1, 9, 9, 9, 2])
    np.testing.assert_array_equal(sc[0, :2], [-1.5, -2.0])
    assert np.isnan(sc[0, 2]) and np.isnan(sc[1, 1:]).all() and sc[1, 0] == -0.25
