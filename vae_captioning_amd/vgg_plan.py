"""Which kernel runs which VGG16 convolution layer, pass and launch: decided once per shape, on the host (no torch, no device).
VggEngine (trainer.py) executes the plan; DESIGN.md section 4 has the table of kernels."""
from collections import namedtuple

from . import spec

ConvLayer = namedtuple("ConvLayer", (
    "name", "H", "W", "cin_eff", "cout", "pooled",   # geometry of the layer's input / output; cin_eff: conv1_1's 3 channels padded to 4
    "fwd_nb", "bwd_nb",          # images per forward / data-gradient launch (the batch, or half of it on two chains)
    "family",                    # forward: "conv1" | "wino4" | "wino2" | "gemm"
    "variant",                   # forward: "mask" (leaves y > 0 as bits) | "pool" (pools, leaves routing codes) | "plain"
    "fwd_v", "fwd_v_bytes",      # forward on the once-transformed input (vc_conv3x3_wino4v_*), and the workspace of that launch
    "bit_words",                 # int32 words of the mask (per chain) or of the routing codes (whole batch); 0: none
    "dgrad",                     # data gradient: "bits" | "plain" (Winograd, ReLU mask from bits / from the activation) | "gemm" | None (conv1_1)
    "dgrad_family",              # "wino4" | "wino2" | None
    "dgrad_v", "dgrad_v_bytes",  # as fwd_v
    "wgrad",                     # weight gradient: "conv1" | "bx" | "wino" | "gemm"
    "pack_fwd", "pack_dgrad",    # elements of the transformed weights in forward / data-gradient order (36 or 16 x Cin x Cout); 0: none
))

ConvPlan = namedtuple("ConvPlan", (
    "layers",           # one ConvLayer per spec.VGG_CONV entry, in order
    "fwd_chains", "bwd_chains",
    "wgrad_ws_bytes",   # workspace of the weight-gradient kernels (full batch, one at a time)
    "tail_ws_bytes",    # (forward, backward): per-chain workspace of the K-split launches of csrc/conv.hip at fwd_nb / bwd_nb images
    "vws_bytes",        # per chain: workspace of the once-transformed input, 0 where the chain has no such launch
))

WINO = {"wino4": "vc_conv3x3_wino4_", "wino2": "vc_conv3x3_wino_"}   # family -> prefix of its library entries
PACK_TAPS = {"wino4": 36, "wino2": 16}


def conv_plan(lib, B, H, W, *, train, chains, precision, use_wino, use_conv1, wino4v, wgrad_bx):
    """The ConvPlan of a forward (+ backward) pass over B images of H x W.

    chains: 1 or 2 half-batch chains, or (forward, backward) where the passes differ (two streams: the backward pass gives its second
    stream to the weight gradients); train: a backward pass follows and wants bits; precision: "f32" | "bf16x3"; use_wino / use_conv1:
    the engine's switches; wino4v: conv4_x / conv5_x on a once-transformed input; wgrad_bx: the direct bf16 weight gradient is allowed.

    Activations between conv1_1 and pool5 are in the C4 layout [B][C/4][H][W][4] (include/vaecap.h).  The rules, each stated here only:
      forward    conv1_1 runs csrc/conv_first.hip ("conv1") where use_conv1, use_wino and vc_conv1_supported at B images.  A layer with
                 Cin % 32 == 0 runs F(4x4,3x3) ("wino4", csrc/conv_wino4.hip) where vc_conv3x3_wino4_preferred at the forward launch
                 batch (every layer of a block between two pools has the same H x W, so a block stays in one family), else F(2x2,3x3)
                 ("wino2", conv_wino.hip) where vc_conv3x3_wino_supported both at one image and at the launch batch.  Everything else --
                 use_wino off, shapes neither takes -- runs the NHWC implicit-GEMM kernels of csrc/conv.hip behind layout conversions
                 ("gemm"; slow, also the independent checker of tests/).
      variant    when training, a Winograd layer that is not pooled and fits one launch leaves its ReLU mask as bits ("mask"), a pooled
                 one pools in its epilogue and leaves MaxPoolGrad's routing codes ("pool").  conv1_1 leaves mask bits when conv1_2 is
                 wino4, H % 16 == 0, W % 16 == 0 and conv1_2's shape fits one launch.
      dgrad      in the family chosen at the forward launch batch where that family supports the data-gradient launch batch, else
                 "gemm"; none when not training.  "bits" only where the layer below left a mask (so it is not pooled) in this family's
                 lane order, both passes launch over the same images (same batch per launch, same number of chains) and the shape fits
                 one launch.
      wino4v     a wino4 launch takes the once-transformed input where wino4v and vc_conv3x3_wino4v_preferred for that launch
                 (wino4v == "fwd": the forward launches only).
      wgrad      conv1_1: "conv1" under the forward's condition.  Cin % 64 == 0 and Cout % 64 == 0 with use_wino: "bx" (csrc/
                 conv_wgrad_bx.hip) in bf16x3 precision where wgrad_bx and supported, else "wino" (F(3x3,2x2), conv_wino_wgrad.hip)
                 where supported.  Else "gemm".
      packs      a layer has transformed weights in forward (data-gradient) order exactly where its forward (data-gradient) family
                 is wino4 or wino2.
    The weight-gradient workspace also covers csrc/conv.hip's kernel for every layer, chosen or not, as it always has: the size is a
    launch argument of all of them."""
    fch, bch = chains if isinstance(chains, tuple) else (chains, chains)
    assert fch in (1, 2) and bch in (1, 2) and (B % 2 == 0 or fch == bch == 1), (B, chains)
    fnb, bnb = B // fch, B // bch
    c1 = bool(use_conv1 and use_wino and lib.vc_conv1_supported(B, H, W))
    geom, h, w = [], H, W
    for name, ci, co in spec.VGG_CONV:
        # the Winograd family of the layer, decided at the forward launch batch
        fam = ("wino4" if lib.vc_conv3x3_wino4_preferred(fnb, h, w, ci, co) else "wino2") if (use_wino and ci % 32 == 0) else None
        geom.append((name, ci, co, h, w, fam))
        if name in spec.VGG_POOL_AFTER:
            h, w = h // 2, w // 2
    layers = []
    wgrad_ws, tail_f, tail_b, vws = lib.vc_conv1_wgrad_workspace_bytes(), 0, 0, [0, 0]
    for li, (name, ci, co, h, w, fam) in enumerate(geom):
        cie, pooled = 4 if ci == 3 else ci, name in spec.VGG_POOL_AFTER
        supported = getattr(lib, WINO[fam] + "supported") if fam else None
        # (wino4_preferred implies wino4_supported at that batch, both directions; wino2 weights are packed only where one image is supported)
        ok = lambda nb, dg: bool(supported(nb, h, w, ci, co, dg)) and (fam == "wino4" or bool(lib.vc_conv3x3_wino_supported(1, h, w, ci, co, dg)))
        family = "conv1" if (ci == 3 and c1) else fam if (fam and ok(fnb, 0)) else "gemm"
        dfam = fam if (fam and train and ok(bnb, 1)) else None
        variant, words = "plain", 0
        if train and family in WINO:
            if pooled:
                variant, words = "pool", lib.vc_conv3x3_wino_pool_words(B, h, w, co)
            elif lib.vc_conv3x3_wino_single_launch_supported(fnb, h, w, cie, co):
                variant, words = "mask", getattr(lib, WINO[family] + "mask_words")(fnb, h, w, co)
        elif (train and family == "conv1" and geom[1][5] == "wino4" and h % 16 == 0 and w % 16 == 0
              and lib.vc_conv3x3_wino_single_launch_supported(fnb, h, w, co, co)):
            variant, words = "mask", lib.vc_conv3x3_wino4_mask_words(fnb, h, w, co)   # bits for conv1_2's F(4x4,3x3) data gradient
        fwd_v = bool(family == "wino4" and wino4v and lib.vc_conv3x3_wino4v_preferred(fnb, h, w, cie, co, 0))
        dgrad_v = bool(dfam == "wino4" and wino4v and wino4v != "fwd" and lib.vc_conv3x3_wino4v_preferred(bnb, h, w, cie, co, 1))
        fwd_vb = lib.vc_conv3x3_wino4v_workspace_bytes(fnb, h, w, cie) if fwd_v else 0
        dgrad_vb = lib.vc_conv3x3_wino4v_workspace_bytes(bnb, h, w, co) if dgrad_v else 0
        if li == 0:
            dgrad = None
        elif dfam is None:
            dgrad = "gemm"
        else:
            below = layers[-1]
            bits = (below.variant == "mask" and (fnb, fch) == (bnb, bch) and dfam == ("wino4" if below.family == "conv1" else below.family)
                    and lib.vc_conv3x3_wino_single_launch_supported(bnb, h, w, cie, co))
            dgrad = "bits" if bits else "plain"
        wide = bool(use_wino and ci % 64 == 0 and co % 64 == 0)
        bx = bool(wide and precision == "bf16x3" and wgrad_bx and lib.vc_conv3x3_bx_wgrad_supported(B, h, w, cie, co))
        wino = bool(wide and lib.vc_conv3x3_wino_wgrad_supported(B, h, w, cie, co))
        wgrad = "conv1" if (ci == 3 and c1) else "bx" if bx else "wino" if wino else "gemm"
        # (csrc/conv.hip's size counts for every layer, a Winograd-path size wherever its kernel could run: see the docstring)
        wgrad_ws = max(wgrad_ws, lib.vc_conv3x3_wgrad_workspace_bytes(B, h, w, cie, co),
                       lib.vc_conv3x3_bx_wgrad_workspace_bytes(B, h, w, cie, co) if bx else 0,
                       lib.vc_conv3x3_wino_wgrad_workspace_bytes(B, h, w, cie, co) if wino else 0)
        tail_f = max(tail_f, lib.vc_conv3x3_fwd_workspace_bytes(fnb, h, w, cie, co), lib.vc_conv3x3_dgrad_workspace_bytes(fnb, h, w, cie, co))
        tail_b = max(tail_b, lib.vc_conv3x3_fwd_workspace_bytes(bnb, h, w, cie, co), lib.vc_conv3x3_dgrad_workspace_bytes(bnb, h, w, cie, co))
        for need, nch in ((fwd_vb, fch), (dgrad_vb, bch)):
            for ch in range(nch):
                vws[ch] = max(vws[ch], need)
        layers.append(ConvLayer(name, h, w, cie, co, pooled, fnb, bnb, family, variant, fwd_v, fwd_vb, words, dgrad, dfam, dgrad_v, dgrad_vb, wgrad,
                                PACK_TAPS[family] * ci * co if family in WINO else 0, PACK_TAPS[dfam] * ci * co if dfam else 0))
    return ConvPlan(tuple(layers), fch, bch, wgrad_ws, (tail_f, tail_b), tuple(vws))
