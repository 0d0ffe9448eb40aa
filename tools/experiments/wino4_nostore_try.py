"""The pooled F(4x4,3x3) forward with and without its full-size output (csrc/conv_wino4.hip, STORE; include/vaecap.h: y == NULL) on the
five pooled VGG16 layers, at the launch size inside the 64-image step (32 images per chain) and at 64.  Per layer and setting: 30 warm
launches timed one by one with HIP events, in alternating groups of five (store, no store, store ...), median and the 10 % / 90 %
quantiles; the pooled tensor and the routing codes of the two settings are compared bit for bit at the timed size.  conv4_3 / conv5_3
also on the once-transformed input (MODE 2).  Run: python tools/experiments/wino4_nostore_try.py [images ...]  (profiles/pool_nostore_layers.txt)"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from vae_captioning_amd import abi  # noqa: E402
from vae_captioning_amd.abi import ptr as P  # noqa: E402

lib = abi.load(os.environ.get("VC_LIB"))
st = lambda: torch.cuda.current_stream().cuda_stream
LAYERS = [("conv1_2", 224, 64, 64), ("conv2_2", 112, 128, 128), ("conv3_3", 56, 256, 256), ("conv4_3", 28, 512, 512), ("conv5_3", 14, 512, 512)]
GROUPS, PER = 6, 5


def one(f):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(); f(); e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


for B in ([int(a) for a in sys.argv[1:]] or [32, 64]):
    print("images %d: pooled forward (bias, ReLU, 2x2 max-pool, routing codes), ms per launch: median [10 %% .. 90 %%] of %d" % (B, GROUPS * PER))
    tot = [0.0, 0.0]
    for name, H, ci, co in LAYERS:
        torch.manual_seed(1)
        x = torch.relu(torch.randn(B, ci // 4, H, H, 4, device="cuda"))
        w = torch.randn(3, 3, ci, co, device="cuda") * (2.0 / (9 * ci)) ** 0.5
        bias = torch.randn(co, device="cuda")
        wp = torch.empty(36 * ci * co, device="cuda")
        lib.vc_conv3x3_wino4_pack_f32(st(), ci, co, P(w), 0, P(wp))
        y = torch.empty(B, co // 4, H, H, 4, device="cuda")
        nw = lib.vc_conv3x3_wino_pool_words(B, H, H, co)
        pl = [torch.zeros(B, co // 4, H // 2, H // 2, 4, device="cuda") for _ in range(2)]
        pb = [torch.zeros(nw, dtype=torch.int32, device="cuda") for _ in range(2)]
        modes = [("fused", None)]
        if lib.vc_conv3x3_wino4v_preferred(B, H, H, ci, co, 0):
            nbytes = lib.vc_conv3x3_wino4v_workspace_bytes(B, H, H, ci)
            modes.append(("MODE 2", (torch.empty(nbytes // 4, device="cuda"), nbytes)))
        for mode, v in modes:
            if v is None:
                f = [lambda: lib.vc_conv3x3_wino4_fwd_pool_f32(st(), B, H, H, ci, co, P(x), P(wp), P(bias), P(y), P(pl[0]), P(pb[0])),
                     lambda: lib.vc_conv3x3_wino4_fwd_pool_f32(st(), B, H, H, ci, co, P(x), P(wp), P(bias), None, P(pl[1]), P(pb[1]))]
            else:
                f = [lambda: lib.vc_conv3x3_wino4v_fwd_pool_f32(st(), B, H, H, ci, co, P(x), P(wp), P(bias), P(y), P(pl[0]), P(pb[0]), P(v[0]), v[1]),
                     lambda: lib.vc_conv3x3_wino4v_fwd_pool_f32(st(), B, H, H, ci, co, P(x), P(wp), P(bias), None, P(pl[1]), P(pb[1]), P(v[0]), v[1])]
            for g in f:
                for _ in range(3):
                    g()
            torch.cuda.synchronize()
            same = torch.equal(pl[0].view(torch.int32), pl[1].view(torch.int32)) and torch.equal(pb[0], pb[1])
            ts = [[], []]
            for _ in range(GROUPS):
                for k in (0, 1):
                    ts[k] += [one(f[k]) for _ in range(PER)]
            q = [np.quantile(t, [0.5, 0.1, 0.9]) for t in ts]
            if v is None:
                tot[0] += q[0][0]; tot[1] += q[1][0]
            print("%-8s %3d %3d->%3d %-6s  with y %.3f [%.3f .. %.3f]  without y %.3f [%.3f .. %.3f]  saved %+.3f ms (%.1f %%)  y = %4.0f MB  pool + codes %s" % (
                name, H, ci, co, mode, q[0][0], q[0][1], q[0][2], q[1][0], q[1][1], q[1][2], q[0][0] - q[1][0], 100 * (q[0][0] - q[1][0]) / q[0][0],
                y.numel() * 4 / 1e6, "bit-identical" if same else "DIFFER"))
            assert same, name
        del x, y, pl, pb
    print("sum of the five fused launches: with y %.3f ms, without %.3f ms, saved %.3f ms" % (tot[0], tot[1], tot[0] - tot[1]))
