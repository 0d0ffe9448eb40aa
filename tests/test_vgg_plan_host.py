"""vgg_plan.conv_plan on the host: the real library's shape queries (pure arithmetic: no device), no torch tensors."""
import itertools

import pytest

from vae_captioning_amd import spec
from vae_captioning_amd.vgg_plan import PACK_TAPS, WINO, conv_plan

GEOMETRIES = [(B, chains) for B in (1, 2, 64, 168) for chains in ((1, 2, (2, 1)) if B % 2 == 0 else (1,))]
SWITCHES = list(itertools.product(("f32", "bf16x3"), (True, False), (True, False)))   # precision, train, use_wino


def build(lib, B, chains, precision, train, use_wino, **kw):
    args = dict(train=train, chains=chains, precision=precision, use_wino=use_wino, use_conv1=True, wino4v=precision == "bf16x3", wgrad_bx=True)
    args.update(kw)
    return conv_plan(lib, B, 224, 224, **args)


@pytest.mark.parametrize("B,chains", GEOMETRIES)
def test_plan_is_complete_consistent_and_covers_the_library_sizes(lib, B, chains):
    for precision, train, use_wino in SWITCHES:
        plan = build(lib, B, chains, precision, train, use_wino)
        assert plan == build(lib, B, chains, precision, train, use_wino)   # equal inputs, equal plans: the cache key is complete
        assert [L.name for L in plan.layers] == [n for n, _, _ in spec.VGG_CONV]
        fch, bch = chains if isinstance(chains, tuple) else (chains, chains)
        assert (plan.fwd_chains, plan.bwd_chains) == (fch, bch)
        H = W = 224
        wgrad_ws, tail, vws = lib.vc_conv1_wgrad_workspace_bytes(), [0, 0], [0, 0]
        for li, ((name, ci, co), L) in enumerate(zip(spec.VGG_CONV, plan.layers)):
            cie = 4 if ci == 3 else ci
            assert (L.H, L.W, L.cin_eff, L.cout, L.pooled) == (H, W, cie, co, name in spec.VGG_POOL_AFTER)
            assert (L.fwd_nb, L.bwd_nb) == (B // fch, B // bch)
            # exactly one choice per pass
            assert L.family in ("conv1", "wino4", "wino2", "gemm") and L.variant in ("mask", "pool", "plain")
            assert L.dgrad in (("bits", "plain", "gemm") if li else (None,)) and L.wgrad in ("conv1", "bx", "wino", "gemm")
            assert (L.family == "conv1") == (ci == 3 and use_wino and bool(lib.vc_conv1_supported(B, H, W)))
            assert (L.wgrad == "conv1") == (L.family == "conv1")
            if not use_wino:
                assert (L.family, L.variant, L.wgrad, L.pack_fwd, L.pack_dgrad) == ("gemm", "plain", "gemm", 0, 0) and L.dgrad in (None, "gemm")
            if not train:
                assert L.variant == "plain" and L.dgrad in (None, "gemm") and not L.bit_words
            # packed copies exactly where the family is Winograd, in that family's size
            assert L.pack_fwd == (PACK_TAPS[L.family] * ci * co if L.family in WINO else 0)
            assert (L.dgrad_family in WINO) == (L.dgrad in ("bits", "plain")) and (L.dgrad_family is None) == (L.dgrad in (None, "gemm"))
            assert L.pack_dgrad == (PACK_TAPS[L.dgrad_family] * ci * co if L.dgrad_family else 0)
            assert L.dgrad_family in (None, L.family)
            # the guards
            if L.family in WINO:
                assert ci % 32 == 0 and getattr(lib, WINO[L.family] + "supported")(L.fwd_nb, H, W, cie, co, 0)
                assert (L.family == "wino4") == bool(lib.vc_conv3x3_wino4_preferred(L.fwd_nb, H, W, ci, co))
            if L.dgrad_family:
                assert getattr(lib, WINO[L.dgrad_family] + "supported")(L.bwd_nb, H, W, cie, co, 1)
            if L.wgrad in ("bx", "wino"):
                assert ci % 64 == 0 and co % 64 == 0
                assert getattr(lib, "vc_conv3x3_%s_wgrad_supported" % {"bx": "bx", "wino": "wino"}[L.wgrad])(B, H, W, cie, co)
            assert (L.wgrad == "bx") <= (precision == "bf16x3")
            # bits only from a mask of the same launch geometry and family
            if L.variant == "mask":
                assert not L.pooled and L.bit_words > 0 and lib.vc_conv3x3_wino_single_launch_supported(L.fwd_nb, H, W, cie if li else co, co)
                if L.family == "conv1":
                    assert H % 16 == 0 and W % 16 == 0 and plan.layers[1].family == "wino4"
                    assert L.bit_words >= lib.vc_conv3x3_wino4_mask_words(L.fwd_nb, H, W, co)
                else:
                    assert L.bit_words >= getattr(lib, WINO[L.family] + "mask_words")(L.fwd_nb, H, W, co)
            if L.variant == "pool":
                assert L.pooled and L.family in WINO and L.bit_words >= lib.vc_conv3x3_wino_pool_words(B, H, W, co)
            if L.dgrad == "bits":
                below = plan.layers[li - 1]
                assert below.variant == "mask" and (below.fwd_nb, fch) == (L.bwd_nb, bch)
                assert L.dgrad_family == ("wino4" if below.family == "conv1" else below.family)
                assert lib.vc_conv3x3_wino_single_launch_supported(L.bwd_nb, H, W, cie, co)
            # the once-transformed input: F(4x4,3x3) launches only, with their workspace
            assert (not L.fwd_v or L.family == "wino4") and (not L.dgrad_v or L.dgrad_family == "wino4")
            if L.fwd_v:
                assert lib.vc_conv3x3_wino4v_supported(L.fwd_nb, H, W, cie, co, 0)
                assert L.fwd_v_bytes >= lib.vc_conv3x3_wino4v_workspace_bytes(L.fwd_nb, H, W, cie) > 0
                vws = [max(v, L.fwd_v_bytes) if ch < fch else v for ch, v in enumerate(vws)]
            if L.dgrad_v:
                assert lib.vc_conv3x3_wino4v_supported(L.bwd_nb, H, W, cie, co, 1)
                assert L.dgrad_v_bytes >= lib.vc_conv3x3_wino4v_workspace_bytes(L.bwd_nb, H, W, co) > 0
                vws = [max(v, L.dgrad_v_bytes) if ch < bch else v for ch, v in enumerate(vws)]
            # what each chosen kernel needs at its launch geometry
            wgrad_ws = max(wgrad_ws, {"conv1": lambda *a: lib.vc_conv1_wgrad_workspace_bytes(), "bx": lib.vc_conv3x3_bx_wgrad_workspace_bytes,
                                      "wino": lib.vc_conv3x3_wino_wgrad_workspace_bytes, "gemm": lib.vc_conv3x3_wgrad_workspace_bytes}[L.wgrad](B, H, W, cie, co))
            if L.family == "gemm":
                tail[0] = max(tail[0], lib.vc_conv3x3_fwd_workspace_bytes(L.fwd_nb, H, W, cie, co))
            if L.dgrad == "gemm":
                tail[1] = max(tail[1], lib.vc_conv3x3_dgrad_workspace_bytes(L.bwd_nb, H, W, cie, co))
            if L.pooled:
                H, W = H // 2, W // 2
        assert plan.wgrad_ws_bytes >= wgrad_ws
        assert plan.tail_ws_bytes[0] >= tail[0] and plan.tail_ws_bytes[1] >= tail[1]
        assert all(p >= v for p, v in zip(plan.vws_bytes, vws))
        assert any(L.fwd_v for L in plan.layers) == (precision == "bf16x3" and use_wino)   # conv4_x / conv5_x


def test_switches_reach_the_plan(lib):
    on = build(lib, 2, 2, "bf16x3", True, True)
    assert {L.wgrad for L in on.layers} == {"conv1", "bx"}
    assert {L.wgrad for L in build(lib, 2, 2, "bf16x3", True, True, wgrad_bx=False).layers} == {"conv1", "wino"}
    assert not any(L.fwd_v or L.dgrad_v for L in build(lib, 2, 2, "bf16x3", True, True, wino4v=False).layers)
    assert build(lib, 2, 2, "f32", True, True, use_conv1=False).layers[0].family == "gemm"
    # the training step: every layer behind conv1_1 on F(4x4,3x3), masks handed down inside each block, routing codes at its end
    for B, chains in ((2, 2), (64, 2)):
        plan = build(lib, B, chains, "f32", True, True)
        assert [L.family for L in plan.layers] == ["conv1"] + ["wino4"] * 12
        assert all(L.variant == ("pool" if L.pooled else "mask") for L in plan.layers)
        assert [L.dgrad for L in plan.layers[1:]] == ["plain" if plan.layers[i].pooled else "bits" for i in range(12)]
    # two streams: the forward pass runs two chains, the backward pass one -- masks of half-batch launches are of no use to it
    plan = build(lib, 2, (2, 1), "f32", True, True)
    assert all(L.dgrad == "plain" for L in plan.layers[1:]) and plan.layers[0].variant == "mask"
