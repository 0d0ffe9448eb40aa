"""The pooled F(4x4,3x3) forward without its full-size output (csrc/conv_wino4.hip, template flag STORE = false; include/vaecap.h: y ==
NULL).  A training step reads only the pooled tensor and MaxPoolGrad's routing codes of a pooled layer (utils/image_embeddings.py:
conv1_2, conv2_2, conv3_3, conv4_3, conv5_3 feed max_pool2d), so the entry may be called with y = NULL and the kernel then has no `out`
path at all.  Only a store disappeared: the pooled tensor must equal the storing call's BIT FOR BIT and the codes word for word, on the
fused kernel (square and linear tile blocks) and on the once-transformed input (MODE 2); the pooled tensor is also held to the fp64
oracle at the family's tolerance (6e-5 of the tensor maximum, flat: tests/test_gpu_conv_wino4.py).

Shapes (B, H, W, Cin, Cout) -- the smallest at which each path can go wrong:
  (1, 16, 16, 64, 32)  square blocks, ONE block (odd count: the second block of the only workgroup is dead), one channel tile
  (2, 32, 32, 64, 96)  square blocks, eight blocks (even), three channel tiles (the chunked workgroup order)
  (3, 14, 14, 64, 64)  conv5's shape: ragged tiles and ragged pooling windows, three blocks (odd)
  (3, 28, 28, 64, 64)  linear tile blocks, 147 tiles = ten blocks (even), the last one partial
  (1, 56, 56, 64, 32)  linear tile blocks, 196 tiles = thirteen blocks (odd), the last one partial
MODE 2 takes every one of them except the 32-wide (its square blocks put tiles in other lanes)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from .gpu_util import P, assert_close, host_c4, stream, zeros

pytestmark = pytest.mark.gpu

from oracle import vgg as OV  # noqa: E402  (checker only)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(1, 16, 16, 64, 32), (2, 32, 32, 64, 96), (3, 14, 14, 64, 64), (3, 28, 28, 64, 64), (1, 56, 56, 64, 32)]
V_SHAPES = [s for s in SHAPES if s[1] != 32]
ids = lambda c: "x".join(map(str, c))
SENTINEL = 0x5a5a5a5a


@pytest.fixture(scope="module")
def data(lib):
    """shape -> inputs on the device, packed weights, the fp64 oracle's pre-activation (computed once, never written)"""
    out = {}
    for case in SHAPES:
        B, H, W, Ci, Co = case
        rng = np.random.default_rng(sum(case) + 17)
        x = np.maximum(rng.standard_normal((B, H, W, Ci), dtype=np.float32), 0)
        w = rng.standard_normal((3, 3, Ci, Co), dtype=np.float32) * np.float32(1 / np.sqrt(9 * Ci))
        b = rng.standard_normal(Co, dtype=np.float32)
        tx, tw, tb = torch.from_numpy(np.ascontiguousarray(x.reshape(B, H, W, Ci // 4, 4).transpose(0, 3, 1, 2, 4))).cuda(), torch.from_numpy(w).cuda(), torch.from_numpy(b).cuda()
        wp = torch.empty(36 * Ci * Co, dtype=torch.float32, device="cuda")
        lib.vc_conv3x3_wino4_pack_f32(stream(), Ci, Co, P(tw), 0, P(wp))
        pre = OV.conv3x3_fwd(x.astype(np.float64), w.astype(np.float64), b.astype(np.float64))
        pre.setflags(write=False)
        out[case] = dict(x=tx, b=tb, wp=wp, pre=pre, bias64=b.astype(np.float64))
    torch.cuda.synchronize()
    return out


def _pooled(a):
    B, H, W, C = a.shape
    return a.reshape(B, H // 2, 2, W // 2, 2, C).max(axis=(2, 4))


def _workspace(lib, case):
    B, H, W, Ci, Co = case
    assert lib.vc_conv3x3_wino4v_supported(B, H, W, Ci, Co, 0) == 1
    nbytes = lib.vc_conv3x3_wino4v_workspace_bytes(B, H, W, Ci)
    return torch.full((nbytes // 4,), float("nan"), dtype=torch.float32, device="cuda"), nbytes


def _fwd_pool(lib, case, d, store, v):
    """-> (y or None, pool, codes) of the pooled forward with routing codes; every output starts from a sentinel"""
    B, H, W, Ci, Co = case
    y = torch.full((B, Co // 4, H, W, 4), float("nan"), device="cuda") if store else None
    pool = torch.full((B, Co // 4, H // 2, W // 2, 4), float("nan"), device="cuda")
    codes = torch.full((lib.vc_conv3x3_wino_pool_words(B, H, W, Co),), SENTINEL, dtype=torch.int32, device="cuda")
    if v:
        vws, nbytes = _workspace(lib, case)
        lib.vc_conv3x3_wino4v_fwd_pool_f32(stream(), B, H, W, Ci, Co, P(d["x"]), P(d["wp"]), P(d["b"]), P(y), P(pool), P(codes), P(vws), nbytes)
    else:
        lib.vc_conv3x3_wino4_fwd_pool_f32(stream(), B, H, W, Ci, Co, P(d["x"]), P(d["wp"]), P(d["b"]), P(y), P(pool), P(codes))
    torch.cuda.synchronize()
    return y, pool, codes


@pytest.mark.parametrize("case", SHAPES, ids=ids)
def test_pooled_forward_without_y_leaves_the_same_pool_and_codes(lib, data, case):
    """fused kernel, relu = 1, codes wanted: y = NULL against a real y, and the pooled tensor once against the fp64 oracle"""
    B, H, W, Ci, Co = case
    d = data[case]
    y1, p1, c1 = _fwd_pool(lib, case, d, True, False)
    y0, p0, c0 = _fwd_pool(lib, case, d, False, False)
    assert y0 is None
    assert torch.equal(p0.view(torch.int32), p1.view(torch.int32)), "pooled tensor differs without y"
    assert torch.equal(c0, c1), "routing codes differ without y"
    assert not torch.isnan(p0).any() and bool((c0 != SENTINEL).any())
    ref = _pooled(np.maximum(d["pre"], 0))
    assert_close(host_c4(p0, (B, H // 2, W // 2, Co)), ref, 6e-5, msg="pooled forward without y vs fp64")
    assert_close(host_c4(y1, (B, H, W, Co)), np.maximum(d["pre"], 0), 6e-5, msg="the storing call's y vs fp64")


@pytest.mark.parametrize("case", V_SHAPES, ids=ids)
def test_pooled_forward_on_the_transformed_input_without_y(lib, data, case):
    """MODE 2 with its workspace: y = NULL against a real y and against the fused kernel without y"""
    d = data[case]
    y1, p1, c1 = _fwd_pool(lib, case, d, True, True)
    y0, p0, c0 = _fwd_pool(lib, case, d, False, True)
    yf, pf, cf = _fwd_pool(lib, case, d, False, False)
    assert torch.equal(p0.view(torch.int32), p1.view(torch.int32)) and torch.equal(c0, c1)
    assert torch.equal(p0.view(torch.int32), pf.view(torch.int32)) and torch.equal(c0, cf)
    assert not torch.isnan(p0).any()


def test_the_32_wide_shape_is_not_one_of_mode_2s(lib):
    assert lib.vc_conv3x3_wino4v_supported(2, 32, 32, 64, 96, 0) == 0


@pytest.mark.parametrize("relu", [0, 1])
@pytest.mark.parametrize("case", SHAPES, ids=ids)
def test_pool_without_codes_and_without_y_for_both_relu_settings(lib, data, case, relu):
    """vc_conv3x3_wino4_fwd_f32 / vc_conv3x3_wino4v_fwd_f32 with ypool: no routing codes (pbits null in the kernel), relu 0 and 1"""
    B, H, W, Ci, Co = case
    d = data[case]
    modes = [False] + ([True] if case in V_SHAPES else [])
    got = []
    for v in modes:
        for store in (True, False):
            y = torch.full((B, Co // 4, H, W, 4), float("nan"), device="cuda") if store else None
            pool = torch.full((B, Co // 4, H // 2, W // 2, 4), float("nan"), device="cuda")
            if v:
                vws, nbytes = _workspace(lib, case)
                lib.vc_conv3x3_wino4v_fwd_f32(stream(), B, H, W, Ci, Co, P(d["x"]), P(d["wp"]), P(d["b"]), P(y), P(pool), relu, P(vws), nbytes)
            else:
                lib.vc_conv3x3_wino4_fwd_f32(stream(), B, H, W, Ci, Co, P(d["x"]), P(d["wp"]), P(d["b"]), P(y), P(pool), relu)
            torch.cuda.synchronize()
            got.append(pool)
    for p in got[1:]:
        assert torch.equal(p.view(torch.int32), got[0].view(torch.int32))
    ref = _pooled(np.maximum(d["pre"], 0) if relu else d["pre"])
    assert_close(host_c4(got[1], (B, H // 2, W // 2, Co)), ref, 6e-5, atol_scale=np.abs(d["pre"]).max(), msg="pool without y, relu %d" % relu)
    if relu:   # the entry with codes leaves the same pooled tensor
        assert torch.equal(_fwd_pool(lib, case, d, False, False)[1].view(torch.int32), got[1].view(torch.int32))
    else:
        assert float(got[1].min()) < 0


def test_no_output_at_all_is_an_argument_error(lib, data):
    """y == NULL needs the pooled tensor: without it nothing is launched (the outputs keep their sentinels) and the call fails"""
    from vae_captioning_amd.abi import VaecapError
    case = SHAPES[0]
    B, H, W, Ci, Co = case
    d = data[case]
    codes = torch.full((lib.vc_conv3x3_wino_pool_words(B, H, W, Co),), SENTINEL, dtype=torch.int32, device="cuda")
    pool = torch.full((B, Co // 4, H // 2, W // 2, 4), float("nan"), device="cuda")
    vws, nbytes = _workspace(lib, case)
    a = (stream(), B, H, W, Ci, Co, P(d["x"]), P(d["wp"]), P(d["b"]))
    with pytest.raises(VaecapError):
        lib.vc_conv3x3_wino4_fwd_pool_f32(*a, None, None, P(codes))
    with pytest.raises(VaecapError):
        lib.vc_conv3x3_wino4v_fwd_pool_f32(*a, None, None, P(codes), P(vws), nbytes)
    with pytest.raises(VaecapError):
        lib.vc_conv3x3_wino4_fwd_pool_f32(*a, None, P(pool), None)       # the codes stay required by this entry
    with pytest.raises(VaecapError):
        lib.vc_conv3x3_wino4_fwd_f32(*a, None, None, 1)
    with pytest.raises(VaecapError):
        lib.vc_conv3x3_wino4v_fwd_f32(*a, None, None, 1, P(vws), nbytes)
    with pytest.raises(VaecapError):
        lib.vc_conv3x3_wino4_fwd_mask_f32(*a, None, 1, P(codes))         # the other entries still need their y
    torch.cuda.synchronize()
    assert bool((codes == SENTINEL).all()) and bool(torch.isnan(pool).all())


def test_a_call_without_y_over_the_launch_limit_is_cut_into_image_ranges(lib, tmp_path):
    """VC_WINO_MAX_BYTES (read once: a fresh process) forces image ranges of 2, 2, 1 on a small shape; the y = NULL call walks them
    without a pointer to offset and leaves what the single launch of this process leaves."""
    B, H, W, Ci, Co = 5, 12, 20, 64, 64
    script = tmp_path / "run.py"
    script.write_text(
        "import sys, numpy as np, torch\n"
        "sys.path.insert(0, %r)\n"
        "from vae_captioning_amd import abi\n"
        "from vae_captioning_amd.abi import ptr as P\n"
        "lib = abi.load(); st = torch.cuda.current_stream().cuda_stream\n"
        "B, H, W, Ci, Co = %d, %d, %d, %d, %d\n"
        "g = torch.Generator(device='cuda').manual_seed(1)\n"
        "x = torch.rand(B, H, W, Ci, device='cuda', generator=g); w = torch.rand(3, 3, Ci, Co, device='cuda', generator=g) - 0.5\n"
        "b = torch.rand(Co, device='cuda', generator=g) - 0.5\n"
        "vp = torch.empty(36 * Ci * Co, device='cuda')\n"
        "lib.vc_conv3x3_wino4_pack_f32(st, Ci, Co, P(w), 0, P(vp))\n"
        "res = {}\n"
        "for tag in ('y', 'n'):\n"
        "    y = torch.zeros(B, H, W, Co, device='cuda') if tag == 'y' else None\n"
        "    yp = torch.zeros(B, H // 2, W // 2, Co, device='cuda'); bits = torch.zeros(lib.vc_conv3x3_wino_pool_words(B, H, W, Co), dtype=torch.int32, device='cuda')\n"
        "    lib.vc_conv3x3_wino4_fwd_pool_f32(st, B, H, W, Ci, Co, P(x), P(vp), P(b), P(y), P(yp), P(bits))\n"
        "    torch.cuda.synchronize()\n"
        "    res['p' + tag] = yp.cpu().numpy(); res['c' + tag] = bits.cpu().numpy()\n"
        "res['single'] = np.array(int(lib.vc_conv3x3_wino_single_launch_supported(B, H, W, Ci, Co)))\n"
        "np.savez(sys.argv[1], **res)\n" % (ROOT, B, H, W, Ci, Co))
    env = dict(os.environ)
    env["VC_WINO_MAX_BYTES"] = str(2 * H * W * 64 * 4)
    f = str(tmp_path / "cut.npz")
    r = subprocess.run([sys.executable, str(script), f], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    cut = np.load(f)
    assert int(cut["single"]) == 0 and lib.vc_conv3x3_wino_single_launch_supported(B, H, W, Ci, Co) == 1
    # the same inputs in this process (one launch)
    g = torch.Generator(device="cuda").manual_seed(1)
    x = torch.rand(B, H, W, Ci, device="cuda", generator=g)
    w = torch.rand(3, 3, Ci, Co, device="cuda", generator=g) - 0.5
    b = torch.rand(Co, device="cuda", generator=g) - 0.5
    vp = torch.empty(36 * Ci * Co, device="cuda")
    lib.vc_conv3x3_wino4_pack_f32(stream(), Ci, Co, P(w), 0, P(vp))
    yp = zeros(B, H // 2, W // 2, Co)
    bits = torch.zeros(lib.vc_conv3x3_wino_pool_words(B, H, W, Co), dtype=torch.int32, device="cuda")
    lib.vc_conv3x3_wino4_fwd_pool_f32(stream(), B, H, W, Ci, Co, P(x), P(vp), P(b), None, P(yp), P(bits))
    torch.cuda.synchronize()
    one_p, one_c = yp.cpu().numpy(), bits.cpu().numpy()
    for k in ("y", "n"):
        assert np.array_equal(cut["p" + k].view(np.int32), one_p.view(np.int32)), k
        assert np.array_equal(cut["c" + k], one_c), k
    assert one_c.any() and np.abs(one_p).max() > 0


STEP_SCRIPT = """
import sys, numpy as np, torch
sys.path.insert(0, %r)
import bench
from vae_captioning_amd import abi, spec, synth
from vae_captioning_amd.trainer import Trainer
B, T, V = 2, bench.T_LEN, bench.VOCAB
p = bench.make_params(dict(bench.WORKLOADS["cfg4"], B=B))
rng = np.random.default_rng(11)
tr = Trainer(p, V, device="cuda", lib=abi.load(), seed=0)
tr.load_state_dict({**spec.init_caption_params(p, V, seed=1), **spec.init_vgg_params(seed=2)})
batch = synth.make_batch(rng, B, p.num_captions, T, V, use_ci=spec.uses_ci(p), images=True, variable_len=True)
noise = synth.make_noise(rng, B * p.num_captions, T, p)
noise["cnn_drop1"] = (rng.random((B, 4096)) < 0.5).astype(np.float32)
noise["cnn_drop2"] = (rng.random((B, 4096)) < 0.5).astype(np.float32)
tr.set_batch(batch, noise)
out = {}
for step in range(2):
    tr.train_step()
    out["losses%%d" %% step] = np.array(tr.losses(), dtype=np.float64)
torch.cuda.synchronize()
params = dict(tr.cap.state_dict())
params.update({n: tr.vgg.store.param(n) for n in tr.vgg.store.names()})
for name in sorted(params):
    out["param__" + bench._dump_name(name)] = bench._dump_sample(name, params[name])
out["has_y"] = np.array([int("y_" + n in tr.vgg.buf) for n in ("conv1_2", "conv2_2", "conv3_3", "conv4_3", "conv5_3", "conv1_1", "conv5_2")])
out["p_none"] = np.array([int(a[1] is None) for a in tr.vgg._acts if a[0] == "P"])
out["peak"] = np.array(torch.cuda.max_memory_allocated())
# whoever asks afterwards still gets the activation of the LAST forward (computed on demand when it was not stored; the optimiser has
# moved the biases since): buf["y_<name>"] and the "P" entries of acts
for (n, x, *_), (nn, *_) in zip(tr.vgg.acts[1:], tr.vgg.acts[:-1]):
    if n == "P":
        assert x is tr.vgg.buf["y_" + nn]
        out["y__" + nn] = bench._dump_sample("y_" + nn, x)
torch.cuda.synchronize()
np.savez(sys.argv[1], **out)
"""


def test_two_training_steps_are_bit_identical_with_and_without_the_store(tmp_path):
    """Trainer at cfg4's configuration (bench.py), 2 images of 224 x 224, fixed weights, injected noise, two steps, in fresh processes
    (the switch is read when the Trainer is built): VC_POOL_STORE_Y=1 against the default.  The losses of both steps and bench.py
    --dump-outputs' sample of every parameter must be equal bit for bit; without the store the five pooled layers have no y_<name>
    after the steps, and reading buf["y_<name>"] / VggEngine.acts afterwards computes the tensor the storing build holds, bit for bit."""
    script = tmp_path / "step.py"
    script.write_text(STEP_SCRIPT % ROOT)
    res = {}
    for mode in ("1", "0"):
        env = dict(os.environ)
        env["VC_POOL_STORE_Y"] = mode
        f = str(tmp_path / ("out%s.npz" % mode))
        r = subprocess.run([sys.executable, str(script), f], env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        res[mode] = np.load(f)
    assert list(res["1"]["has_y"]) == [1, 1, 1, 1, 1, 1, 1] and list(res["0"]["has_y"]) == [0, 0, 0, 0, 0, 1, 1]
    assert list(res["1"]["p_none"]) == [0] * 5 and list(res["0"]["p_none"]) == [1] * 5
    print("peak device memory at 2 images: store %d bytes, no store %d bytes" % (int(res["1"]["peak"]), int(res["0"]["peak"])))
    keys = sorted(k for k in res["1"].files if k.startswith(("losses", "param__", "y__")))
    assert len(keys) > 35 and sorted(k for k in res["0"].files if k.startswith(("losses", "param__", "y__"))) == keys
    assert sum(k.startswith("y__") for k in keys) == 5 and all(np.abs(res["0"][k]).max() > 0 for k in keys if k.startswith("y__"))
    for k in keys:
        a, b = res["1"][k], res["0"][k]
        assert a.dtype == b.dtype and a.tobytes() == b.tobytes(), k
    assert np.isfinite(res["0"]["losses1"]).all() and not np.array_equal(res["0"]["losses0"], res["0"]["losses1"])
    assert int(res["0"]["peak"]) < int(res["1"]["peak"])
