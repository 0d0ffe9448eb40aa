"""VGG16 engine + the training-step harness (counterpart of main.py:186-290's inner loop).

Data parallelism (new work, the reference is single-GPU): one process per GPU,
replicated parameters, the minibatch sharded by image; ONE RCCL all-reduce per step over
the single flat gradient buffer (caption-side grads | reduction scalars | VGG grads),
plus a 4-byte all-reduce of the non-PAD token count that the CE gradient scale needs
before backward (main.py:156-157 divides by the GLOBAL count).
"""
import contextlib
import os

import numpy as np
import torch

from . import abi, spec
from .abi import ptr as P
from .engine import EMA_SUFFIX, TAIL, CaptionEngine, FlatStore, _stream, ema_omd, internal_caption_variables, split_averages, _round
from .vgg_plan import WINO, conv_plan


def imagenet_weights(weight_file):
    """{cnn/* variable name: float32 array} from a vgg16_weights.npz, by the reference's rule
    (utils/image_embeddings.py:240-246, quirk Q18): the first 30 ALPHABETICALLY SORTED arrays (conv1_1_W, conv1_1_b ...
    conv5_3_b, fc6_W, fc6_b, fc7_W, fc7_b) are assigned to `parameters` in creation order; fc8_* are skipped."""
    names = [n for n, _ in spec.vgg_variables()]
    out = {}
    with np.load(weight_file) as w:
        for i, k in enumerate(sorted(w.keys())):
            if i == 30:
                break
            out[names[i]] = np.ascontiguousarray(w[k], dtype=np.float32)
    return out


class _EngineBuffers(dict):
    """VggEngine.buf: name -> tensor.  Reading buf["y_<name>"] of a pooled layer whose full-size activation the last forward did
    not store (VggEngine.pool_store_y) computes it then (VggEngine._materialise); `in` and .get() do not."""

    def __init__(self, engine):
        dict.__init__(self)
        self._engine = engine

    def __missing__(self, key):
        t = self._engine._materialise(key)
        if t is None:
            raise KeyError(key)
        return t


class VggEngine(object):
    """utils/image_embeddings.py:26-238 on device: 13 x (conv3x3 + bias + ReLU), 5 max-pools,
    fc1 / fc2 (+ dropout), forward and backward, plus cnn_optimizer (ops/optimizers.py:49-82)."""

    def __init__(self, p, device="cuda", lib=None, grad_backing=None, seed=0, rank=0):
        self.p = p
        self.lib = lib or abi.load()
        self.dev = device
        self.store = FlatStore(spec.vgg_variables(), device, tail=0, grad_backing=grad_backing)
        self.buf = _EngineBuffers(self)
        self._acts = []      # the last forward's (layer name, input tensor, H, W, Cin_eff, Cout, weights used): what backward() walks
        self._dropped = {}   # pooled layer whose y_<name> the last forward did not store -> what _materialise needs to compute it
        self.ws = None
        self.ws_bytes = 0
        self.tail_ws = {}
        self.train = bool(p.fine_tune) and p.mode == "training"
        self.keep = float(p.cnn_dropout) if self.train else 1.0  # main.py:67-73
        self.wd = float(p.weight_decay) if self.train else 0.0
        self.seed, self.rank = seed, rank
        self.inject = False
        self.timer = None
        self.precision = "f32"   # "bf16x3": fc1 / fc2 products and the weight gradients on the bf16 pipe (per call, like CaptionEngine.precision)
        # the weight gradient of layer l and the data-gradient chain (layer l, then l-1 ...) are independent:
        # wgrads run on a side stream so that the tail of one kernel (the last partial round of workgroups)
        # is filled by the other instead of idling the chip
        # Convolution dispatch: which kernel runs which layer, pass and launch is decided once per shape by vgg_plan.conv_plan (the rules are
        # in its docstring, the table of kernels in DESIGN.md section 4); forward / backward / _pack_weights execute the plan of self._plan
        self.use_conv1 = True
        # False: a layer whose plan variant is "pool" gets no full-size activation -- y_<name> is not allocated, the pooled forward is
        # called with y = NULL (csrc/conv_wino4.hip compiles the whole `out` path away) and the layer's "P" entry of self._acts carries
        # None.  Nothing in a training step reads that tensor: the next layer and its weight gradient read p_<name>, MaxPoolGrad +
        # ReluGrad the routing codes, the data gradient behind a pool has no ReLU source (1.57 GB of HBM writes and of device memory
        # per 64-image step).  Whoever wants it afterwards (checkers, tools) reads buf["y_<name>"] or self.acts as before and gets it
        # computed on demand from what the forward kept (_materialise): the step pays five bias copies of <= 2 KB for that.  An engine
        # driven by hand stores every activation in its forward; the Trainer switches the store off (VC_POOL_STORE_Y=1 keeps it: A/B runs).
        self.pool_store_y = True
        self.use_wino = os.environ.get("VC_CONV_WINO", "1") != "0"
        # conv4_x / conv5_x forward + data gradient on a once-transformed input (csrc/conv_wino4.hip MODE 2; bit-identical to the fused
        # kernel).  Measured inside the cfg4 step (profiles/r06_wino4v_step.md): the main kernels shrink by 15-25 % but the 24 transform
        # launches per step sit on the chains; f32 25.85-25.93 ms against 25.81-25.88 fused (nothing), split-bf16 mode 21.39 against
        # 21.66 (its shorter weight-gradient stream leaves the chains critical).  Default: on in the split-bf16 mode only; VC_WINO4V=1 / 0 forces.
        # The FORWARD alone is another matter: it has no third stream beside its two chains, so what its kernels save comes off the step
        # (profiles/pool_nostore_bench.md: 25.49-25.53 ms with MODE 2 on the forward of conv4_x / conv5_x only against 25.65-25.72 fused).
        # wino4v_f32 is the f32 default: False for an engine driven by hand, "fwd" (forward launches only, vgg_plan.conv_plan) in the
        # Trainer, on whose step that was measured; VC_WINO4V=fwd / 1 / 0 forces.
        self.wino4v_f32 = False
        self._wino4v_env = os.environ.get("VC_WINO4V")
        self.vws = {}   # conv chain -> workspace of the transformed input
        # split-bf16 mode (this engine's precision): the direct weight gradient on the bf16 matrix pipe (csrc/conv_wgrad_bx.hip) replaces
        # the f32 Winograd F(3x3,2x2) kernel (VC_WGRAD_BX=0: A/B runs)
        self.wgrad_bx = os.environ.get("VC_WGRAD_BX", "1") != "0"
        self._plans = {}   # conv_plan's inputs -> ConvPlan
        # Streams: 3 = two half-batch convolution chains + the weight gradients on a third stream (the tail of one launch is filled by
        # another stream's launch; the data-parallel gradient buckets are issued from the weight-gradient stream), 1 = serial
        nstreams = int(os.environ.get("VC_VGG_STREAMS", "3"))
        self._side = torch.cuda.Stream() if nstreams >= 2 else None
        self._side2 = torch.cuda.Stream() if nstreams >= 3 else None
        # Trainer.capture() sets this: a hipGraph capture of the backward pass's stream pattern (the weight-gradient stream waiting
        # for the chain streams layer after layer) crashes in hipStreamEndCapture (ROCm 7.2); forward-only captures are fine.  A
        # captured step therefore runs the VGG16 on the caller's stream alone.
        self.one_stream = False
        self.part = torch.zeros(self.lib.vc_sumsq_blocks(), dtype=torch.float32, device=device)
        # sum(w^2) of the regulariser: the Adam update of step t leaves the per-workgroup sums of the NEW parameters, which are step t + 1's
        # w (0.16 ms per step saved: no second pass over 0.54 GB); invalid after any other write to the parameters
        # fc1 / fc2 (the tail of the flat buffer, 89 % of it) may be updated before the convolution layers: two launches, each
        # leaving its own per-block sums of w^2
        self.o_fc = self.store.offset("cnn/fc1/weights")
        self.w2_blocks = (self.lib.vc_adam_blocks(self.o_fc), self.lib.vc_adam_blocks(self.store.n - self.o_fc))
        self.w2_part = torch.zeros(sum(self.w2_blocks), dtype=torch.float32, device=device)
        self.w2_valid = False
        self.w2_cache = True     # False: always recompute sum(w^2) (a captured step: parameters restored behind the graph's back would go unnoticed)
        self._w2_version = -1
        # Weight averaging (CaptionEngine.ema_decay): only a VGG16 that is trained has averages.  `step` is the device step counter
        # the warm-up reads (the caption engine's: the Trainer hands it over); ema_warmup as CaptionEngine.ema_warmup.
        self.ema_decay, self.ema_omd = ema_omd(getattr(p, "ema_decay", 0.0) if self.train else 0.0)
        self.ema_warmup = True
        self.step = None
        if self.ema_decay > 0:
            self.store.slot("ema").copy_(self.store.p)

    @property
    def side(self):
        return None if self.one_stream else self._side

    @property
    def side2(self):
        return None if self.one_stream else self._side2

    def _b(self, name, shape, dtype=torch.float32):
        t = self.buf.get(name)
        shape = tuple(int(s) for s in shape)
        if t is None or tuple(t.shape) != shape or t.dtype != dtype:
            t = torch.zeros(shape, dtype=dtype, device=self.dev)
            self.buf[name] = t
            # the zero-fill is enqueued on the current stream: the side streams must not touch the new
            # buffer before it has run (first step only; buffers persist afterwards)
            cur = torch.cuda.current_stream()
            for s in (self.side, self.side2):
                if s is not None and s != cur:
                    s.wait_stream(cur)
        return t

    @property
    def acts(self):
        """The last forward's (layer name, input tensor, H, W, Cin_eff, Cout, weights used) for whoever inspects it: like _acts, with
        the input of a "P" entry that the forward did not store (pool_store_y) computed now (buf["y_<name>"])."""
        out = []
        for i, a in enumerate(self._acts):
            if a[0] == "P" and a[1] is None:
                a = (a[0], self.buf["y_" + self._acts[i - 1][0]]) + tuple(a[2:])
            out.append(a)
        return out

    def _materialise(self, key):
        """buf["y_<name>"] of a pooled layer whose full-size activation the last forward did not store: the plain F(4x4,3x3) forward
        of that layer over the same image ranges, on its retained input, this step's packed weights and the bias as it was -- the
        same accumulators and epilogue arithmetic as the pooled launch, so exactly the tensor a storing forward leaves.  Enqueued on
        the caller's stream, which the forward joined with its side streams before it returned; dropped again by the next forward."""
        name = key[2:] if key.startswith("y_") else None
        if name not in self._dropped:
            return None
        x, H, W, cie, co, ranges, bias = self._dropped[name]
        y = self._b(key, (x.shape[0], co // 4, H, W, 4))
        for b0, nb in ranges:
            self.lib.vc_conv3x3_wino4_fwd_f32(_stream(), nb, H, W, cie, co, P(x[b0:]), P(dict.__getitem__(self.buf, "vp_" + name)), P(bias), P(y[b0:]), None, 1)
        return y

    def _need_ws(self, nbytes):
        if nbytes > self.ws_bytes:
            self.ws = torch.empty(max(int(nbytes), 1 << 20) // 4 + 16, dtype=torch.float32, device=self.dev)
            self.ws_bytes = self.ws.numel() * 4

    def _chain_ws(self, i, nb, need):
        """Workspace of conv chain i (one per stream: chains run concurrently) for the K-split tail launches of the
        forward / data-gradient convolutions at nb images: `need` bytes (ConvPlan.tail_ws_bytes)."""
        key = (i, nb)
        t = self.tail_ws.get(key)
        if t is None:
            t = self.tail_ws[key] = torch.empty(max(need, 16) // 4 + 16, dtype=torch.float32, device=self.dev)
        return t

    def _plan(self, B, H, W):
        """The ConvPlan of a pass over B images of H x W under the engine's current switches (they may change between steps)."""
        fch = 2 if (self.side is not None and B % 2 == 0 and B >= 2) else 1
        bch = 2 if (self.side2 is not None and B % 2 == 0) else 1   # (with two streams the second one takes the weight gradients)
        key = (B, H, W, self.train, (fch, bch), self.precision, self.use_wino, self.use_conv1, self.use_wino4v, self.wgrad_bx)
        plan = self._plans.get(key)
        if plan is None:
            B, H, W, train, chains, precision, use_wino, use_conv1, wino4v, wgrad_bx = key
            plan = self._plans[key] = conv_plan(self.lib, B, H, W, train=train, chains=chains, precision=precision, use_wino=use_wino,
                                                use_conv1=use_conv1, wino4v=wino4v, wgrad_bx=wgrad_bx)
        for ch, need in enumerate(plan.vws_bytes):
            if need and (ch not in self.vws or self.vws[ch].numel() * 4 < need):
                self.vws[ch] = torch.empty(need // 4, dtype=torch.float32, device=self.dev)
        return plan

    def gemm(self, ta, tb, M, N, K, A, lda, B, ldb, C, ldc, bias=None, flags=0):
        self._need_ws(self.lib.vc_gemm_workspace_bytes(M, N, K))
        self.lib.vc_gemm_f32(_stream(), ta, tb, M, N, K, P(A), lda, P(B), ldb, P(C), ldc, P(bias), flags | (4 if self.precision == "bf16x3" else 0),
                             P(self.ws), self.ws_bytes)

    def _timed(self, tag, flops, fn):
        if self.timer is not None:
            self.timer.run(tag, flops, fn)
        else:
            fn()

    def _pack_weights(self, plan):
        """Transformed (G g G^T) copies of the 3x3 kernels in the Winograd kernels' operand order (forward layout, and the flipped
        + transposed one of the data gradient when a backward pass follows), for the layers whose plan asks for them.  Runs on the
        weight-gradient stream, which is idle during the forward pass: the forward copies first, in layer order, each followed by
        the event its layer's launches wait for (returned as {layer: event}), then the data-gradient copies, which only the
        backward pass waits for (self.packed_bwd)."""
        self.packed_bwd = None
        if not self.use_wino:
            return {}
        lib, S = self.lib, self.store
        main = torch.cuda.current_stream()
        st = self.side2 if self.side2 is not None else (self.side if self.side is not None else main)
        if st != main:
            st.wait_stream(main)
        evs = {}
        self._pack_events = evs   # (kept alive for the step: a hipGraph capture holds their records)
        with torch.cuda.stream(st):
            sh = _stream()
            for dgrad in ((0, 1) if self.train else (0,)):
                for L in plan.layers:
                    fam, n = (L.dgrad_family, L.pack_dgrad) if dgrad else (L.family, L.pack_fwd)
                    if n:
                        w = S.param(spec.vgg_var_names(L.name)[0])
                        getattr(lib, WINO[fam] + "pack_f32")(sh, L.cin_eff, L.cout, P(w), dgrad, P(self._b(("vpt_" if dgrad else "vp_") + L.name, (n,))))
                        if not dgrad:
                            evs[L.name] = torch.cuda.Event()
                            evs[L.name].record(torch.cuda.current_stream())
            if self.train:
                self.packed_bwd = torch.cuda.Event()
                self.packed_bwd.record(torch.cuda.current_stream())
        return evs

    @property
    def use_wino4v(self):
        if self._wino4v_env == "fwd":   # (A/B runs: the forward launches only, the data gradient stays fused -- vgg_plan.conv_plan)
            return "fwd"
        if self._wino4v_env is not None:
            return self._wino4v_env != "0"
        return True if self.precision == "bf16x3" else self.wino4v_f32

    def _wino(self, family, entry, v, ch):
        """-> (the entry `entry` ("fwd_mask_f32", "dgrad_bits_f32" ...) of a Winograd family, its trailing arguments).  v: the launch
        runs on a once-transformed input -- the F(4x4,3x3) entry of the same name with chain ch's transform workspace appended
        (bit-identical results, same mask bits: csrc/conv_wino4.hip MODE 2)."""
        if v:
            ws = self.vws[ch]
            return getattr(self.lib, "vc_conv3x3_wino4v_" + entry), (P(ws), ws.numel() * 4)
        return getattr(self.lib, WINO[family] + entry), ()

    def colsum(self, x, rows, cols, out):
        self._need_ws(self.lib.vc_colsum_workspace_bytes(rows, cols))
        self.lib.vc_colsum_f32(_stream(), P(x), rows, cols, cols, P(out), 0, P(self.ws), self.ws_bytes)

    def load_params(self, named):
        missing = [n for n in self.store.names() if n not in named]
        if missing:  # tf.train.Saver.restore raises NotFoundError for the same situation
            raise KeyError("checkpoint lacks %d cnn/* variable(s), e.g. %s -- it was written without the VGG16 variables" % (len(missing), missing[0]))
        self.w2_valid = False
        self._load_into(self.store.param, named)
        if self.ema_decay > 0:   # the averages start from the parameters (warm-up on) unless the dict carries them
            self.store.slot("ema").copy_(self.store.p)
            avg = {k: v for k, v in split_averages(named).items() if k.startswith("cnn/")}
            lacking = [n for n in self.store.names() if n not in avg]
            if avg and lacking:
                raise KeyError("checkpoint carries averaged cnn/* weights but lacks %d of them, e.g. %s%s" % (len(lacking), lacking[0], EMA_SUFFIX))
            self.ema_warmup = not avg
            if avg:
                self._load_into(self.store.average, avg)

    def _load_into(self, view, named):
        for name in self.store.names():
            dst = view(name)
            if tuple(np.shape(named[name])) != tuple(dst.shape):
                raise ValueError("%s: checkpoint shape %s, model shape %s" % (name, tuple(np.shape(named[name])), tuple(dst.shape)))
            dst.copy_(torch.from_numpy(np.ascontiguousarray(named[name], dtype=np.float32)))

    def load_weights(self, weight_file):
        """utils/image_embeddings.py:240-246: first 30 alphabetically sorted npz arrays."""
        self.w2_valid = False
        for name, arr in imagenet_weights(weight_file).items():
            self.store.param(name).copy_(torch.from_numpy(arr))
        if self.ema_decay > 0:
            self.store.slot("ema").copy_(self.store.p)
            self.ema_warmup = True

    def state_dict(self):
        torch.cuda.synchronize()
        return {n: self.store.param(n).detach().cpu().numpy().copy() for n in self.store.names()}

    def averages_dict(self):
        """The moving averages of the cnn/* variables by name; needs ema_decay > 0."""
        torch.cuda.synchronize()
        return {n: self.store.average(n).detach().cpu().numpy().copy() for n in self.store.names()}

    def grads_dict(self):
        torch.cuda.synchronize()
        return {n: self.store.grad(n).detach().cpu().numpy().copy() for n in self.store.names()}

    def set_masks(self, drop1, drop2):
        self.inject = True
        for k, a in (("drop1", drop1), ("drop2", drop2)):
            self._b(k, a.shape).copy_(torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)))

    # ------------------------------------------------------------------ forward
    def _to_nhwc(self, tag, t, nb, H, W, C):
        """NHWC copy of the C4 tensor t (fallback path: the kernels of csrc/conv.hip are NHWC)."""
        out = self._b("nhwc_" + tag, (nb, H, W, C))
        self.lib.vc_c4_to_nhwc_f32(_stream(), nb, H, W, C, P(t), P(out))
        return out

    def forward(self, images, step=None):
        """images [B, 224, 224, 3] float32 RGB 0..255 on device -> fc2 [B, 4096]."""
        lib, st, S = self.lib, _stream(), self.store
        B, H, W = int(images.shape[0]), int(images.shape[1]), int(images.shape[2])
        self.B = B
        x = self._b("x0", (B, H, W, 4))   # NHWC4 == C4 with one channel quad
        if images.dtype == torch.uint8:
            lib.vc_vgg_preprocess_u8(st, P(images), B, H, W, P(x))
        else:
            lib.vc_vgg_preprocess_f32(st, P(images), B, H, W, P(x))
        plan = self.plan = self._plan(B, H, W)
        c1 = plan.layers[0].family == "conv1"   # conv1_1 through csrc/conv_first.hip (unpadded weights)
        w4 = self._b("w1_4", (3, 3, 4, 64))
        if not c1:
            lib.vc_pad_dim_f32(st, P(S.param("cnn/conv1_1/weights")), 9, 3, 4, 64, P(w4))
        packed = self._pack_weights(plan)
        self._acts = []  # (layer name, input tensor, H, W, Cin_eff, Cout, weights used)
        for gone in self._dropped:   # (an activation somebody asked for after the previous forward is that forward's, not this one's)
            self.buf.pop("y_" + gone, None)
        self._dropped = {}
        # The conv / pool chain of one image is independent of every other image: with two streams the
        # batch is pushed through as two half-batch chains so that the tail of each kernel (its last partial
        # round of workgroups) overlaps the other chain's kernels.  Halves are contiguous slices of the leading (image) dimension.
        main = torch.cuda.current_stream()
        side = self.side if plan.fwd_chains == 2 else None
        halves = [(0, B // 2, main), (B // 2, B // 2, side)] if side is not None else [(0, B, main)]
        if side is not None:
            side.wait_stream(main)
        for L in plan.layers:
            name, cie, co, pooled = L.name, L.cin_eff, L.cout, L.pooled
            wn, bn = spec.vgg_var_names(name)
            w = w4 if cie == 4 else S.param(wn)
            # (the pooled F(4x4,3x3) forward of a training step leaves the pooled tensor and the routing codes only: pool_store_y)
            drop_y = L.variant == "pool" and L.family == "wino4" and not self.pool_store_y
            y = None if drop_y else self._b("y_" + name, (B, co // 4, H, W, 4))
            if drop_y:   # what _materialise needs: the input (kept anyway), the launch ranges, and the bias as it is NOW (the optimiser moves it)
                bias_now = self._b("bias_" + name, (co,))
                bias_now.copy_(S.param(bn))
                self._dropped[name] = (x, H, W, cie, co, [(b0, nb) for b0, nb, _ in halves], bias_now)
            yp = self._b("p_" + name, (B, co // 4, H // 2, W // 2, 4)) if pooled else None
            # pooled layer in training: the 2x2 max-pool is register math in the epilogue; it also leaves MaxPoolGrad's routing codes (4 bits
            # per pooled element), so the backward pass does not re-read the pre-pool activation
            pool_bits = self._b("pb_" + name, (L.bit_words,), dtype=torch.int32) if L.variant == "pool" else None
            for ch, (b0, nb, strm) in enumerate(halves):
                tws = self._chain_ws(ch, nb, plan.tail_ws_bytes[0])
                with torch.cuda.stream(strm):
                    sh = _stream()
                    fl = 2.0 * nb * H * W * 9 * (3 if cie == 4 else cie) * co
                    # "mask": the next layer is a convolution on this output -- leave (y > 0) as bits in the lane order of ITS data gradient
                    # (conv1_1: conv1_2's F(4x4,3x3) data gradient), per tile of THIS launch geometry
                    mk = self._b("mk_%s_%d" % (name, ch), (L.bit_words,), dtype=torch.int32) if L.variant == "mask" else None
                    if L.family == "conv1":  # conv1_1: its own HBM-bound kernel, unpadded weights
                        if mk is not None:
                            self._timed("conv_fwd", fl, lambda: lib.vc_conv1_fwd_mask_f32(sh, nb, H, W, P(x[b0:]), P(S.param(wn)), P(S.param(bn)), P(y[b0:]), P(mk)))
                        else:
                            self._timed("conv_fwd", fl, lambda: lib.vc_conv1_fwd_f32(sh, nb, H, W, P(x[b0:]), P(S.param(wn)), P(S.param(bn)), P(y[b0:]), 1))
                    elif L.family in WINO:   # Winograd (calls over 2 GiB are cut into image ranges inside the library)
                        torch.cuda.current_stream().wait_event(packed[name])   # this layer's transformed weights of this step are ready
                        if L.variant == "mask":
                            out = (P(y[b0:]), 1, P(mk))
                        elif L.variant == "pool":
                            out = (P(y[b0:]) if y is not None else None, P(yp[b0:]), P(pool_bits[b0 * (H // 2) * (W // 2) * (co // 8):]))
                        else:
                            out = (P(y[b0:]), P(yp[b0:]) if pooled else None, 1)
                        fn, va = self._wino(L.family, {"mask": "fwd_mask_f32", "pool": "fwd_pool_f32", "plain": "fwd_f32"}[L.variant], L.fwd_v, ch)
                        self._timed("conv_fwd", fl, lambda: fn(sh, nb, H, W, cie, co, P(x[b0:]), P(self.buf["vp_" + name]), P(S.param(bn)), *out, *va))
                    else:
                        # NHWC implicit-GEMM kernels of csrc/conv.hip behind layout conversions: any shape (VC_CONV_WINO=0, odd image sizes)
                        xn = self._to_nhwc("x_%s_%d" % (name, ch), x[b0:], nb, H, W, cie)   # (buffers keyed by layer: a shared name would be re-allocated at every shape change)
                        yn = self._b("nhwc_y_%s_%d" % (name, ch), (nb, H, W, co))
                        self._timed("conv_fwd", fl, lambda: lib.vc_conv3x3_fwd_f32(
                            sh, nb, H, W, cie, co, P(xn), P(w), P(S.param(bn)), P(yn), 1, P(tws), tws.numel() * 4))
                        lib.vc_nhwc_to_c4_f32(sh, nb, H, W, co, P(yn), P(y[b0:]))
                        if pooled:   # (B * co / 4 planes of H x W four-channel pixels: the NHWC kernel on C4 data)
                            lib.vc_maxpool2x2_fwd_f32(sh, nb * (co // 4), H, W, 4, P(y[b0:]), P(yp[b0:]))
            self._acts.append((name, x, H, W, cie, co, w))
            x = y
            if pooled:
                self._acts.append(("P", x, H, W, co, co, pool_bits))
                x = yp
                H, W = H // 2, W // 2
        if side is not None:
            main.wait_stream(side)
        # pool5 in the reference's order: [B, 7, 7, 512] NHWC == [B, 25088] (image_embeddings.py:222); 6.4 MB at 64 images
        co = int(x.shape[1]) * 4
        self.pool5 = x
        flat = self._b("flat", (B, H, W, co))
        lib.vc_c4_to_nhwc_f32(st, B, H, W, co, P(x), P(flat))
        self.flat = flat
        F1 = H * W * co
        fc1 = self._b("fc1", (B, 4096))
        fc1_bytes = 4.0 * (F1 * 4096 + B * F1 + B * 4096)   # the weight matrix (411 MB) + both activations: the product is HBM-bound at B <= 64
        self._timed("hbm_fc1_gemm", fc1_bytes,
                    lambda: self.gemm(0, 0, B, 4096, F1, flat, F1, S.param("cnn/fc1/weights"), 4096, fc1, 4096, S.param("cnn/fc1/biases"), 1))
        fc2 = self._b("fc2", (B, 4096))
        if self.keep < 1:
            if not self.inject:
                for i, k in enumerate(("drop1", "drop2")):
                    m = self._b(k, (B, 4096))
                    lib.vc_philox_bernoulli_f32(st, P(m), m.numel(), self.keep, self.seed * 1000003 + self.rank, (8 + i) << 32, P(step))
            fc1d = self._b("fc1d", (B, 4096))
            lib.vc_dropout_f32(st, P(fc1), P(self.buf["drop1"]), self.keep, B * 4096, P(fc1d))
        else:
            fc1d = fc1
        self.fc1d = fc1d
        self.gemm(0, 0, B, 4096, 4096, fc1d, 4096, S.param("cnn/fc2/weights"), 4096, fc2, 4096, S.param("cnn/fc2/biases"), 1)
        if self.keep < 1:
            fc2d = self._b("fc2d", (B, 4096))
            lib.vc_dropout_f32(st, P(fc2), P(self.buf["drop2"]), self.keep, B * 4096, P(fc2d))
        else:
            fc2d = fc2
        return fc2d

    def reg_sumsq(self, out_ptr):
        """sum(w^2) over every cnn/* variable (main.py:69-74, Q9: biases included) -> device scalar."""
        lib, st = self.lib, _stream()
        # the partial sums the previous step's Adam update left are good only while nobody else has written the parameters: torch
        # bumps the flat buffer's version counter on every in-place write through it or a view of it (load_state_dict, p.copy_, ...),
        # the library's own kernels do not
        if self.w2_valid and self.w2_cache and self.store.p._version == self._w2_version:
            lib.vc_reduce_sum_f32(st, P(self.w2_part), self.w2_part.numel(), 1.0, out_ptr, 0)
            return
        lib.vc_sumsq_partial_f32(st, P(self.store.p), self.store.n, P(self.part))
        lib.vc_reduce_sum_f32(st, P(self.part), self.part.numel(), 1.0, out_ptr, 0)

    # ------------------------------------------------------------------ backward
    def backward(self, dfc2, after_fc=None, after_layer=None):
        """after_fc: optional callback invoked as soon as the fc1 / fc2 gradients (89 % of the VGG
        gradient bytes) are final, so their all-reduce can overlap the convolution backward.
        after_layer: optional (conv layer name, callback): invoked on the weight-gradient stream right after
        that layer's weight gradient has been enqueued (every gradient of that layer and of the layers
        above it is then final in stream order)."""
        lib, st, S = self.lib, _stream(), self.store
        B = self.B
        m1 = P(self.buf["drop1"]) if self.keep < 1 else None
        m2 = P(self.buf["drop2"]) if self.keep < 1 else None
        d2 = self._b("d_fc2", (B, 4096))
        lib.vc_relu_bwd_f32(st, P(dfc2), P(self.buf["fc2"]), m2, self.keep, B * 4096, P(d2))
        self.gemm(1, 0, 4096, 4096, B, self.fc1d, 4096, d2, 4096, S.grad("cnn/fc2/weights"), 4096)
        self.colsum(d2, B, 4096, S.grad("cnn/fc2/biases"))
        d1 = self._b("d_fc1", (B, 4096))
        self.gemm(0, 1, B, 4096, 4096, d2, 4096, S.param("cnn/fc2/weights"), 4096, d1, 4096)
        lib.vc_relu_bwd_f32(st, P(d1), P(self.buf["fc1"]), m1, self.keep, B * 4096, P(d1))
        F1 = self.flat.numel() // B
        fc1_bytes = 4.0 * (F1 * 4096 + B * F1 + B * 4096)
        self._timed("hbm_fc1_gemm_bwd", fc1_bytes, lambda: self.gemm(1, 0, F1, 4096, B, self.flat, F1, d1, 4096, S.grad("cnn/fc1/weights"), 4096))
        self.colsum(d1, B, 4096, S.grad("cnn/fc1/biases"))
        dn = self._b("d_pool5", tuple(self.flat.shape))
        self._timed("hbm_fc1_gemm_bwd", fc1_bytes, lambda: self.gemm(0, 1, B, F1, 4096, d1, 4096, S.param("cnn/fc1/weights"), 4096, dn, F1))
        d = self._b("d_pool5_c4", tuple(self.pool5.shape))   # back into the convolution layers' C4 layout
        lib.vc_nhwc_to_c4_f32(st, B, int(dn.shape[1]), int(dn.shape[2]), int(dn.shape[3]), P(dn), P(d))
        if after_fc is not None:
            after_fc()
        dw4 = self._b("dw1_4", (3, 3, 4, 64))
        plan = self.plan
        layer = {L.name: L for L in plan.layers}
        self._need_ws(plan.wgrad_ws_bytes)
        main = torch.cuda.current_stream()
        side, side2 = self.side, self.side2
        # streams: with 3, the data-gradient chain runs as two half-batch chains (main, side) and every
        # weight gradient (full batch) on side2; with 2, one full-batch chain (main) + weight gradients (side)
        split = plan.bwd_chains == 2
        wst = side2 if split else side
        halves = [(0, B // 2, main), (B // 2, B // 2, side)] if split else [(0, B, main)]
        if self.packed_bwd is not None:   # the data-gradient weight copies made during the forward pass
            main.wait_event(self.packed_bwd)
        if split:
            side.wait_stream(main)
        for li in range(len(self._acts) - 1, -1, -1):
            name, x, H, W, ci, co, w = self._acts[li]
            if name == "P":
                dx = self._b("dx_%d" % li, (B, co // 4, H, W, 4))
                for b0, nb, strm in halves:
                    with torch.cuda.stream(strm):  # + ReluGrad of the conv that made x
                        if w is not None:   # routing codes from the pooled Winograd forward: no read of x
                            lib.vc_maxpool2x2_bwd_bits_f32(_stream(), nb, H, W, co, P(w[b0 * (H // 2) * (W // 2) * (co // 8):]), P(d[b0:]), P(dx[b0:]))
                        else:   # (planes of four-channel pixels: the NHWC kernel on C4 data)
                            lib.vc_maxpool2x2_bwd_f32(_stream(), nb * (co // 4), H, W, 4, P(x[b0:]), P(d[b0:]), P(dx[b0:]), 1)
                d = dx
                continue
            L = layer[name]
            wn, bn = spec.vgg_var_names(name)
            cr = 3 if ci == 4 else ci  # algorithmic channel count (conv1_1 is zero-padded 3 -> 4)
            fl = 2.0 * B * H * W * 9 * cr * co

            def wgrad(L=L, x=x, d=d, wn=wn, bn=bn, ci=ci, co=co, H=H, W=W, fl=fl):
                sw = _stream()
                if L.wgrad == "conv1":
                    self._timed("conv_wgrad", fl, lambda: lib.vc_conv1_wgrad_f32(sw, B, H, W, P(x), P(d), P(S.grad(wn)), P(S.grad(bn)), 0, P(self.ws), self.ws_bytes))
                elif L.wgrad == "gemm":   # csrc/conv.hip on NHWC copies (conv1_1: zero-padded 4-channel weights)
                    xn, dn_ = self._to_nhwc("wx_" + wn, x, B, H, W, ci), self._to_nhwc("wd_" + wn, d, B, H, W, co)
                    self._timed("conv_wgrad", fl, lambda: lib.vc_conv3x3_wgrad_f32(sw, B, H, W, ci, co, P(xn), P(dn_), P(dw4 if ci == 4 else S.grad(wn)), P(S.grad(bn)), 0,
                                                                                   P(self.ws), self.ws_bytes))
                    if ci == 4:
                        lib.vc_pad_dim_f32(sw, P(dw4), 9, 4, 3, 64, P(S.grad(wn)))
                else:
                    # "bx": split-bf16 mode, direct, K = the pixels, operands split in registers
                    # "wino": Winograd F(3x3,2x2), both operands transformed in registers, K = the 2x2 tiles
                    fn = {"bx": lib.vc_conv3x3_bx_wgrad_f32, "wino": lib.vc_conv3x3_wino_wgrad_f32}[L.wgrad]
                    self._timed("conv_wgrad", fl, lambda: fn(sw, B, H, W, ci, co, P(x), P(d), P(S.grad(wn)), P(S.grad(bn)), 0, P(self.ws), self.ws_bytes))
            if wst is not None:
                wst.wait_stream(main)  # d (this layer's pre-activation gradient) is final on the chain stream(s)
                if split:
                    wst.wait_stream(side)
                with torch.cuda.stream(wst):
                    wgrad()
                    if after_layer is not None and after_layer[0] == name:
                        after_layer[1]()
            else:
                wgrad()
                if after_layer is not None and after_layer[0] == name:
                    after_layer[1]()
            if li > 0:
                prev_is_pool = self._acts[li - 1][0] == "P"
                dx = self._b("dx_%d" % li, (B, ci // 4, H, W, 4))
                for ch, (b0, nb, strm) in enumerate(halves):
                    tws = self._chain_ws(ch, nb, plan.tail_ws_bytes[1])
                    with torch.cuda.stream(strm):
                        sh = _stream()
                        if L.dgrad == "gemm":   # csrc/conv.hip on NHWC copies
                            dn_ = self._to_nhwc("d_%s_%d" % (name, ch), d[b0:], nb, H, W, co)
                            xn = None if prev_is_pool else self._to_nhwc("x_%s_%d" % (name, ch), x[b0:], nb, H, W, ci)
                            dxn = self._b("nhwc_dx_%s_%d" % (name, ch), (nb, H, W, ci))
                            self._timed("conv_dgrad", fl * nb / B, lambda: lib.vc_conv3x3_dgrad_f32(
                                sh, nb, H, W, ci, co, P(dn_), P(w), P(xn), P(dxn), P(tws), tws.numel() * 4))
                            lib.vc_nhwc_to_c4_f32(sh, nb, H, W, ci, P(dxn), P(dx[b0:]))
                            continue
                        if L.dgrad == "bits":
                            # ReluGrad from the bits the previous layer's forward left (one 8-byte load per lane instead of sixteen 16-byte ones)
                            relu = P(self.buf["mk_%s_%d" % (self._acts[li - 1][0], ch)])
                        else:
                            relu = None if prev_is_pool else P(x[b0:])
                        fn, va = self._wino(L.dgrad_family, {"bits": "dgrad_bits_f32", "plain": "dgrad_f32"}[L.dgrad], L.dgrad_v, ch)
                        self._timed("conv_dgrad", fl * nb / B, lambda: fn(sh, nb, H, W, ci, co, P(d[b0:]), P(self.buf["vpt_" + name]), relu, P(dx[b0:]), *va))
                d = dx
        if split:
            main.wait_stream(side)
        if wst is not None:
            main.wait_stream(wst)

    def apply_gradients(self, scal, part=None):
        """cnn_optimizer: no clipping; Adam(cnn_lr, beta1=0.8) by default; the L2 regulariser's
        gradient wd*w is folded into the update.  part: None = every cnn/* variable; "fc" = fc1 + fc2 only (their gradients are
        final as soon as the fc backward has run: the caller may update them on another stream under the convolution backward);
        "conv" = the convolution layers only.  The update is elementwise, so the two halves equal the whole."""
        p, lib, st, S = self.p, self.lib, _stream(), self.store
        ema = self.ema_decay > 0
        if ema:
            if self.ema_warmup and self.step is None:
                raise RuntimeError("weight averaging with its warm-up reads the device step counter: set VggEngine.step (the Trainer does)")
            e_args = (self.ema_omd, P(self.step) if self.ema_warmup else None)
        for which, lo, n, w2o in (("conv", 0, self.o_fc, 0), ("fc", self.o_fc, S.n - self.o_fc, self.w2_blocks[0])):
            if part is not None and part != which:
                continue
            sl = lambda t: t.data_ptr() + lo * 4
            if p.cnn_optimizer == "Adam" and ema:   # the average of this part's range [lo, lo + n) inside the update's own pass
                if self.wd:
                    self._timed("hbm_adam", 36.0 * n, lambda: lib.vc_adam_sumsq_ema_f32(
                        st, sl(S.p), sl(S.g), sl(S.slot("m")), sl(S.slot("v")), sl(S.slot("ema")), n, scal.data_ptr() + 12, None, 0.8, 0.999, 1e-8,
                        self.wd, *e_args, self.w2_part.data_ptr() + w2o * 4))
                else:
                    self._timed("hbm_adam", 36.0 * n, lambda: lib.vc_adam_ema_f32(
                        st, sl(S.p), sl(S.g), sl(S.slot("m")), sl(S.slot("v")), sl(S.slot("ema")), n, scal.data_ptr() + 12, None, 0.8, 0.999, 1e-8,
                        self.wd, *e_args))
            elif p.cnn_optimizer == "Adam" and self.wd:
                self._timed("hbm_adam", 28.0 * n, lambda: lib.vc_adam_sumsq_f32(
                    st, sl(S.p), sl(S.g), sl(S.slot("m")), sl(S.slot("v")), n, scal.data_ptr() + 12, None, 0.8, 0.999, 1e-8, self.wd,
                    self.w2_part.data_ptr() + w2o * 4))
            elif p.cnn_optimizer == "Adam":
                self._timed("hbm_adam", 28.0 * n, lambda: lib.vc_adam_f32(
                    st, sl(S.p), sl(S.g), sl(S.slot("m")), sl(S.slot("v")), n, scal.data_ptr() + 12, None, 0.8, 0.999, 1e-8, self.wd))
            elif p.cnn_optimizer == "SGD":
                lib.vc_sgd_f32(st, sl(S.p), sl(S.g), n, scal.data_ptr() + 16, None, self.wd)
            else:
                lib.vc_momentum_f32(st, sl(S.p), sl(S.g), sl(S.slot("a")), n, scal.data_ptr() + 16, None, 0.9, self.wd, None, 0)
            if ema and p.cnn_optimizer != "Adam":
                lib.vc_ema_update_f32(st, sl(S.slot("ema")), sl(S.p), n, *e_args)
        # (every block of both halves has written its sum by the time the next forward pass reads them, whatever the order)
        self.w2_valid = p.cnn_optimizer == "Adam" and bool(self.wd)
        self._w2_version = self.store.p._version


class _NoPending(object):
    """Handle of a muted collective (Trainer.mute_collectives)."""

    def wait(self):
        pass


class Trainer(object):
    """One training step = main.py:241-244's sess.run([kld, rec_loss, lower_bound, optimize,
    optimize_cnn, annealing])."""

    def __init__(self, p, vocab, device="cuda", lib=None, world=1, rank=0, group=None, seed=0, force_collectives=False, comm="auto",
                 wgrad_stream=True, precision=None):
        """wgrad_stream: weight gradients of the caption side, its clip + optimiser and fc1 / fc2's optimiser run on a second
        stream (under the LSTM recurrences and the VGG16 backward pass); False = everything in program order on one stream --
        the same kernels on the same data either way, so the results are bit-identical.
        comm: how the data-parallel collectives run.  "abi" = libvaecap's own RCCL entries (dp.AbiComm: vc_allreduce_sum_f32 ...);
        "torch" = torch.distributed on `group`; "auto" = "abi" when the collectives are on and the process group is RCCL-backed
        (backend "nccl") or there is no process group at all (one forced rank), "torch" otherwise (the gloo test path).
        An existing dp.AbiComm may be passed instead."""
        self.p, self.lib = p, (lib or abi.load())
        # precision: "f32" (default: the reference's tf.float32 arithmetic) or "bf16x3" (split-bf16 operands, three bf16 MFMAs, f32
        # accumulate: every dense product of the step, the LSTM recurrences and the VGG16 weight gradients -- an opt-in mode with ~1e-5
        # relative product error, reported on its own bench lines, never the default).  None = VC_PRECISION, else "f32".  The mode
        # belongs to THIS trainer: its engines pass it with every library call (ABI 4), no process-wide state is read or written.
        precision = precision or os.environ.get("VC_PRECISION") or "f32"
        if precision not in ("f32", "bf16x3"):
            raise ValueError("precision must be 'f32' or 'bf16x3', not %r" % (precision,))
        self.precision = precision
        self.collectives = world > 1 or force_collectives
        self.world, self.rank, self.group = world, rank, group
        self.dev = device
        n_cap = sum(_round(int(np.prod(s))) for _, s in internal_caption_variables(p, vocab)) + TAIL
        self.fine = bool(p.fine_tune)
        n_vgg = sum(_round(int(np.prod(s))) for _, s in spec.vgg_variables()) if self.fine else 0
        self.gall = torch.zeros(n_cap + n_vgg, dtype=torch.float32, device=device)  # THE all-reduce buffer
        self.cap = CaptionEngine(p, vocab, device, self.lib, grad_backing=self.gall[:n_cap], world=world, rank=rank, group=group, seed=seed,
                                 force_collectives=force_collectives)
        self.cap.set_precision(self.precision)
        self.cap.enable_wgrad_stream(bool(wgrad_stream) and os.environ.get("VC_WGRAD_STREAM", "1") != "0")   # (VC_WGRAD_STREAM=0: A/B runs)
        self.vgg = None
        if self.fine:
            self.vgg = VggEngine(p, device, self.lib, grad_backing=self.gall[n_cap:], seed=seed, rank=rank)
            self.vgg.precision = self.precision
            self.vgg.step = self.cap.step   # (weight averaging: the warm-up of the cnn/* averages reads the one step counter)
            self.vgg.pool_store_y = os.environ.get("VC_POOL_STORE_Y", "0") == "1"   # (VggEngine.pool_store_y; 1: A/B runs, checkers that read y_<name>)
            self.vgg.wino4v_f32 = "fwd"   # (VggEngine.wino4v_f32: the f32 forward of conv4_x / conv5_x on the once-transformed input)
            if self.vgg.wd:
                self.cap.reg_scale = self.vgg.wd / 2.0  # l2_regularizer(wd)(w) = wd * sum(w^2)/2
        self.images = None
        self.graph = None
        self.dp_stats = None  # list: per-bucket (index, bytes, event before wait, event after wait) when bench.py asks for it
        self.cnn_host = None  # {cnn/* name: array} written into checkpoints when VGG16 is not on device (state_dict)
        self.n_cap = n_cap
        self.ema_decay = self.cap.ema_decay   # weight averaging (DESIGN.md "Weight averaging"); 0 = off
        self._ema_swapped = False             # inside `with self.ema_weights()`
        # Data-parallel gradient exchange.  Logically ONE sum-all-reduce of `gall` per step; with VGG
        # fine-tuning it is issued as four asynchronous pieces in the order the gradients become final
        # (caption side | fc1+fc2, 478 MB | conv3_1..conv5_3, 58 MB | conv1_1..conv2_2, 1 MB) so that RCCL
        # overlaps the convolution backward and only the last megabyte is exposed
        # (VC_DP_BUCKETS=0 forces the single blocking call).
        self.buckets = os.environ.get("VC_DP_BUCKETS", "1") != "0"
        self.off_fc = n_cap + self.vgg.store.offset("cnn/fc1/weights") if self.vgg is not None else None
        self.off_c3 = n_cap + self.vgg.store.offset("cnn/conv3_1/weights") if self.vgg is not None else None
        self.comm = None
        self.trace = os.environ.get("VC_TRACE", "0") == "1" and bool(self.lib.vc_trace_available())
        self._open_range = False
        if self.collectives:
            self._setup_comm(comm)

    def _setup_comm(self, comm):
        import torch.distributed as dist
        from . import dp
        if isinstance(comm, dp.AbiComm):
            self.comm = comm
        else:
            if comm == "auto":
                env = os.environ.get("VC_DP_COMM", "")
                if env in ("abi", "torch"):
                    comm = env
                elif dist.is_available() and dist.is_initialized():
                    comm = "abi" if dist.get_backend(self.group) == "nccl" else "torch"
                else:
                    comm = "abi" if self.world == 1 else "torch"
            if comm == "abi":
                dev = torch.cuda.current_device()
                if self.world == 1:
                    self.comm = dp.AbiComm.single(self.lib, dev)
                else:
                    self.comm = self._agree_on_abi_comm(dev)
        if self.comm is not None:   # the engine's collective hooks go through the C ABI
            self.cap.reduce_fn, self.cap.gather_fn, self.cap.rscatter_fn = self.comm.all_reduce, self.comm.all_gather, self.comm.reduce_scatter

    def _agree_on_abi_comm(self, dev):
        """The libvaecap communicator for world > 1, or None with every rank on torch.distributed -- the ranks must end up on the
        SAME path whatever fails where, so each stage is agreed on through the process group before the next one starts:
          1. vc_comm_available() on every rank (an RCCL library can be bound);
          2. rank 0 creates the unique id and broadcasts it -- or the error text -- to the group (broadcast_object_list: the group's
             own transport, no private store, nobody waits on a key that never appears);
          3. ncclCommInitRank on every rank (RCCL refuses e.g. two ranks on one GPU: an error on all of them), then a last MIN.
        (A rank that dies INSIDE the collective init still hangs the others -- that is RCCL's contract, not something a handshake
        in front of it can repair.)"""
        import torch.distributed as dist
        from . import dp
        on_gpu = dist.get_backend(self.group) == "nccl"

        def all_ok(ok):
            flag = torch.tensor([1.0 if ok else 0.0], device="cuda" if on_gpu else "cpu")
            dist.all_reduce(flag, op=dist.ReduceOp.MIN, group=self.group)
            return float(flag.item()) == 1.0

        def give_up(why):
            if self.rank == 0:
                print("libvaecap communicator not available on every rank (%s): collectives through torch.distributed" % why, flush=True)
            return None
        if not all_ok(bool(self.lib.vc_comm_available())):
            return give_up("no RCCL library could be bound on some rank")
        msg = [None]
        if self.rank == 0:
            try:
                msg = [("id", dp.AbiComm.unique_id(self.lib))]
            except abi.VaecapError as e:
                msg = [("error", str(e))]
        src = dist.get_global_rank(self.group, 0) if self.group is not None else 0
        dist.broadcast_object_list(msg, src=src, group=self.group)
        if msg[0][0] != "id":
            return give_up(msg[0][1])
        comm, err = None, None
        try:
            comm = dp.AbiComm(self.lib, self.world, self.rank, dev, msg[0][1])
        except abi.VaecapError as e:
            err = e
        if not all_ok(err is None):
            if comm is not None:
                comm.destroy()
            return give_up(err or "another rank failed")
        return comm

    def set_batch(self, batch, noise=None):
        extra = []
        if self.fine:
            img = np.asarray(batch["images"])
            # uint8 pixels (what the reference's HDF5 holds, preprocess.py:27-28) travel as bytes -- 9.6 MB instead of 38.5 MB per 64
            # images -- and are cast on the device (vc_vgg_preprocess_u8); anything else is fed as float32 like the placeholder's cast
            extra = [("images", img, torch.uint8)] if img.dtype == np.uint8 else [("images", np.asarray(img, np.float32), torch.float32)]
        self.cap.set_batch(batch, noise, extra=extra)  # one pinned staging buffer, one asynchronous copy
        if self.fine:
            self.images = self.cap.buf["images"]
            if noise is not None and "cnn_drop1" in noise:
                self.vgg.set_masks(noise["cnn_drop1"], noise["cnn_drop2"])

    def _range(self, name):
        """roctx range around a phase of the step (VC_TRACE=1; `rocprofv3 --marker-trace`); name None closes the open range."""
        if self.trace:
            if self._open_range:
                self.lib.vc_trace_pop()
            if name is not None:
                self.lib.vc_trace_push(name.encode())
            self._open_range = name is not None

    def _step(self):
        cap, vgg = self.cap, self.vgg
        feats = None
        if vgg is not None:
            self._range("vgg16_forward")
            feats = vgg.forward(self.images, cap.step)
            if vgg.wd:
                vgg.reg_sumsq(cap.red.data_ptr() + 12)
        self._range("caption_forward")
        cap.forward(feats)
        self._range("caption_backward")
        dfe = cap.backward(want_dfeatures=vgg is not None)
        # Weight gradients, the clip and the optimisers are off the gradient chain (cap.off_chain: the weight-gradient stream when
        # Trainer has enabled it, else this stream): the caption side's run under the VGG16 backward pass, fc1 / fc2's Adam under
        # the convolution layers' backward.  Collectives keep their order: caption bucket, fc, conv3_1.., conv1_1..
        with cap.off_chain():
            cap.pack_tail()
        fine = vgg is not None and vgg.train
        self._range("vgg16_backward+allreduce" if fine else "allreduce")
        if self.collectives and self.buckets and fine and self.reduce_async_fn is not None:
            from . import dp
            bk = dp.gradient_buckets(self.n_cap, self.gall.numel(), self.off_fc, self.off_c3)
            issue = lambda i: self.reduce_async_fn(self.gall[bk[i][0]:bk[i][1]])

            def wait(i, h):
                if self.dp_stats is not None:  # how long the waiting stream stalls on each bucket (bench.py reports it)
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    h.wait()
                    e1.record()
                    self.dp_stats.append((i, (bk[i][1] - bk[i][0]) * 4, e0, e1))
                else:
                    h.wait()

            def fc_final():
                with cap.off_chain():
                    wait(1, issue(1))
                    vgg.apply_gradients(cap.scal, "fc")

            pending = []
            with cap.off_chain():
                wait(0, issue(0))
                cap.apply_gradients()
            vgg.backward(dfe, after_fc=fc_final, after_layer=("conv3_1", lambda: pending.append((2, issue(2)))))
            pending.append((3, issue(3)))
            for i, h in pending:
                wait(i, h)
            self._range("optimizers")
            vgg.apply_gradients(cap.scal, "conv")
        else:
            if self.collectives:
                if fine:
                    vgg.backward(dfe)
                cap.join_off_chain()
                self.all_reduce_grads()  # the single gradient all-reduce (RCCL over xGMI)
                self._range("optimizers")
                with cap.off_chain():
                    cap.apply_gradients()
                if fine:
                    vgg.apply_gradients(cap.scal)
            else:
                with cap.off_chain():
                    cap.apply_gradients()
                if fine:
                    def fc_final():
                        with cap.off_chain():
                            vgg.apply_gradients(cap.scal, "fc")
                    vgg.backward(dfe, after_fc=fc_final)
                    self._range("optimizers")
                    vgg.apply_gradients(cap.scal, "conv")
        cap.join_off_chain()
        self._range(None)

    @property
    def reduce_async_fn(self):
        if getattr(self.cap, "_fake_collectives", False):
            return None
        if getattr(self, "_muted", False):   # mute_collectives: same bucket / stream structure, nothing on the wire
            return lambda t: _NoPending()
        if self.comm is not None:
            return self.comm.all_reduce_async
        return lambda t: torch.distributed.all_reduce(t, group=self.group, async_op=True)

    def mute_collectives(self):
        """Replace every collective of the step by a no-op (timing only: bench.py measures the compute-only step to report the
        exposed communication time = step - compute-only step).  The step keeps its structure -- the four gradient pieces are still
        "issued" and "waited for" where the real ones are, so the optimisers overlap the VGG16 backward pass exactly as in the real
        step.  Returns the function that restores the collectives."""
        cap = self.cap
        saved = (cap.reduce_fn, cap.gather_fn, cap.rscatter_fn)
        cap.reduce_fn = lambda t: None
        cap.gather_fn = lambda out, inp: out.view(self.world, -1).copy_(inp.view(1, -1).expand(self.world, -1))
        cap.rscatter_fn = lambda out, inp: out.copy_(inp.view(-1)[:out.numel()].view_as(out))
        self._muted = True

        def restore():
            cap.reduce_fn, cap.gather_fn, cap.rscatter_fn = saved
            self._muted = False
        return restore

    def all_reduce_grads(self):
        if self.collectives:
            self.cap.reduce_fn(self.gall)  # the single gradient all-reduce (RCCL over xGMI)

    def train_step(self):
        if self._ema_swapped:
            raise RuntimeError("no training step inside ema_weights(): the parameters and their averages have changed places")
        if self.graph is not None:
            self.graph.replay()
            self.cap.param_updates += 1   # the replayed optimiser kernels rewrote the parameters (CaptionEngine.param_version)
        else:
            self._step()

    # ------------------------------------------------------------------ self-critical training (scst.py; DESIGN.md "Self-critical training")
    def enable_scst(self, reward, bos, eos, baseline="average", beta=0.0, max_len=None):
        """Make scst_step available.  reward: any object with rewards(candidates_per_image, references_per_image) -> float64 per
        candidate (scst.CiderReward, scst.RougeReward, a scst.SumReward of them); baseline: "average" (the image's other samples) or "greedy" (the
        greedy decode under the same z); beta: weight of the token-entropy bonus (>= 0); max_len: longest sample (default gen_max_len)."""
        from . import scst
        from .generate import CaptionGenerator
        p = self.p
        if self.fine:
            raise RuntimeError("self-critical training does not train the VGG16: not with --fine_tune")
        if self.ema_decay > 0:
            raise RuntimeError("self-critical training updates ranges of the store only: not with --ema_decay")
        if self.collectives:
            raise RuntimeError("self-critical training is single-GPU: not in a data-parallel run")
        if p.mode != "training":
            raise RuntimeError("self-critical training needs --mode training")
        if float(p.temperature) != 1.0:
            raise ValueError("self-critical training samples at temperature 1: the policy gradient needs the probabilities of the "
                             "distribution that was sampled (got %r)" % (p.temperature,))
        scst.check_baseline(baseline, p.num_captions)
        if not (0.0 <= float(beta) < float("inf")):
            raise ValueError("the entropy weight must be finite and >= 0 (got %r)" % (beta,))
        self.scst = dict(reward=reward, bos=int(bos), eos=int(eos), baseline=baseline, beta=float(beta), max_len=int(max_len or p.gen_max_len),
                         gen=CaptionGenerator(self.cap))
        self.scst_stats = None
        self.scst_times = None   # a dict: scst_step adds the host-clock seconds of its phases (tools/scst_time.py; synchronises per phase)

    def scst_sample(self, batch, method="sample", eps=None, uniforms=None):
        """The K = num_captions captions of every image of `batch` decoded under K prior draws: -> (per image its K candidates
        (tokens incl. <EOS> when ended, logprob, ended) in draw order, i.e. caption row b*K + k; the z rows [B*K, S, L] they were decoded
        under -- the sampler's own device buffer, valid until its next pass; None without an encoder).
        eps [K, S, B, L] / uniforms [K, max_len, B]: injected draws (Philox on the device step counter when None: a "greedy" pass that
        follows a "sample" pass of the same step decodes under the same z)."""
        from .engine import K_CL
        sc, p, cap = self.scst, self.p, self.cap
        gen, K = sc["gen"], int(p.num_captions)
        feats = np.asarray(batch["features"], np.float32)
        B = feats.shape[0]
        if B * K > gen.diverse_rows:
            raise ValueError("%d images x %d samples exceed the sampler's %d rows per pass" % (B, K, gen.diverse_rows))
        c_v = np.asarray(batch["c_v"], np.float32).reshape(B, K, K_CL)[:, 0] if cap.use_ci else None   # (batches carry c_v tiled to rows)
        _, cands = gen._diverse_pass(feats, c_v, eps, K, method, sc["bos"], sc["eos"], sc["max_len"], 0.7, None, uniforms, 4)
        return cands, (gen.buf["dvi%d_%d_z" % (B, K)] if cap.enc else None)

    def policy_step(self, adv, z=None, beta=0.0):
        """One policy-gradient step on the uploaded batch of sampled captions (CaptionEngine.policy_forward / backward(policy) /
        policy_apply_gradients), with the step's off-chain structure: weight gradients, clip and optimiser on the weight-gradient stream."""
        cap = self.cap
        if self.graph is not None:
            raise RuntimeError("a trainer whose step was captured into a hipGraph cannot run policy steps (the graph bakes the XE step's inputs)")
        import time
        times = getattr(self, "scst_times", None)   # (a dict: this step's phases on the host clock, each closed by a device synchronise)
        t0 = time.perf_counter()
        self._range("policy_forward")
        cap.policy_forward(adv, z, beta)
        self._range("policy_backward")
        cap.backward(policy=True)
        with cap.off_chain():
            cap.pack_tail()
        if times is not None:
            cap.join_off_chain()
            torch.cuda.synchronize()
            times["policy_fwd_bwd"] = times.get("policy_fwd_bwd", 0.0) + time.perf_counter() - t0
            t0 = time.perf_counter()
        self._range("optimizers")
        with cap.off_chain():
            cap.policy_apply_gradients()
        cap.join_off_chain()
        self._range(None)
        if times is not None:
            torch.cuda.synchronize()
            times["optimiser"] = times.get("optimiser", 0.0) + time.perf_counter() - t0

    def scst_step(self, batch, noise=None, eps=None, uniforms=None):
        """One self-critical step on an XE batch (features [B, F], cap_enc / lengths: the images' human captions = the references,
        c_v): sample, (greedy baseline), rewards -> advantages, policy step.  noise: injected decoder dropout masks of the policy
        forward (drop_in / drop_out, [T, N, .] with T = the longest sample -- tests); eps / uniforms: injected draws of the sampler.
        Returns (and keeps in self.scst_stats) reward (mean sampled reward), baseline (mean baseline reward), sample_len, ended_share,
        entropy (mean token entropy, None with beta == 0), logprob (mean log-probability of a sample under the policy forward)."""
        import time
        from . import scst
        sc, p, cap = self.scst, self.p, self.cap
        K = int(p.num_captions)
        times = self.scst_times

        def lap(name, t0):
            if times is not None and name is not None:
                torch.cuda.synchronize()
                times[name] = times.get(name, 0.0) + time.perf_counter() - t0
            return time.perf_counter()
        t = lap(None, 0.0)
        cands, z = self.scst_sample(batch, "sample", eps, uniforms)
        if z is not None:
            z = z.clone()   # (the greedy pass runs through the same sampler buffers; equal values, but the step keeps its own copy)
        t = lap("sample", t)
        B = len(cands)
        samples = [list(c[0]) for cs in cands for c in cs]
        refs = scst.batch_references(batch["cap_enc"], batch["lengths"], K)
        g = None
        if sc["baseline"] == "greedy":
            gc, _ = self.scst_sample(batch, "greedy", eps, None)
            t = lap("greedy", t)
            g = sc["reward"].rewards([[c[0] for c in cs] for cs in gc], refs).reshape(B, K)
        r = sc["reward"].rewards([[c[0] for c in cs] for cs in cands], refs).reshape(B, K)
        adv = scst.advantages(r, sc["baseline"], g)
        t = lap("reward", t)
        pb = scst.policy_batch(samples, sc["bos"], sc["eos"])
        pb["features"] = batch["features"]
        if cap.use_ci:
            pb["c_v"] = batch["c_v"]
        self.set_batch(pb, noise)
        t = lap("upload", t)
        self.policy_step(adv.reshape(-1).astype(np.float32), z, sc["beta"])
        ps = cap.policy_stats()
        self.scst_stats = dict(reward=float(r.mean()), baseline=float((r - adv).mean()), sample_len=float(pb["lengths"].mean()),
                               ended_share=float(np.mean([c[2] for cs in cands for c in cs])), entropy=ps["entropy"], logprob=ps["logprob"])
        return self.scst_stats

    def capture(self, warmup=2):
        """Capture the whole step into one hipGraph (removes ~300 launch latencies per step).
        Requires fixed shapes and device-generated noise; collectives stay outside graphs."""
        assert not self.collectives and not self.cap.inject
        self.cap.fix_inputs()   # the graph bakes input addresses: later set_batch calls copy INTO these persistent tensors
        if self.fine:
            self.images = self.cap.buf["images"]
        if self.vgg is not None:
            self.vgg.w2_cache = False
            self.vgg.one_stream = True   # (see VggEngine.__init__; the buffers of the one-chain geometry are made by the un-captured steps below)
            warmup = max(warmup, 1)
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            for _ in range(warmup):
                self._step()
        torch.cuda.current_stream().wait_stream(s)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            self._step()
        self.graph = g

    def eval_rec_loss(self):
        """validate() of main.py:262-284: rec_loss of the TRAINING graph (dropout active, z ~ q)."""
        cap, vgg = self.cap, self.vgg
        feats = vgg.forward(self.images, cap.step) if vgg is not None else None
        cap.forward(feats, train=False)
        return cap.losses()[1]

    def losses(self):
        return self.cap.losses()

    def objective_stats(self):
        return self.cap.objective_stats()

    def sched_stats(self):
        return self.cap.sched_stats()

    # ------------------------------------------------------------------ checkpoints
    def state_dict(self):
        """Every trainable variable of the reference graph (main.py:186-191).  The reference builds the VGG16 variables
        even when it trains on precomputed features (on a dummy input, with the ImageNet weights loaded "for further
        usage", main.py:63-66,205-208, quirk Q22), so its checkpoints always carry cnn/*: without --fine_tune they come
        from `cnn_host` (set by main.py from the ImageNet npz, or kept from the checkpoint that was restored)."""
        d = self.cap.state_dict()
        if self.vgg is not None:
            d.update(self.vgg.state_dict())
        elif self.cnn_host is not None:
            d.update(self.cnn_host)
        # weight averaging: <name>/ExponentialMovingAverage beside every TRAINED variable (the cnn_host constants have none)
        for eng in self._ema_engines():
            d.update({k + EMA_SUFFIX: v for k, v in eng.averages_dict().items()})
        return d

    # ------------------------------------------------------------------ weight averaging (DESIGN.md "Weight averaging")
    def _ema_engines(self):
        """The engines whose store has the slot "ema": the caption side with ema_decay > 0, and the VGG16 when it is trained as well."""
        return [e for e in (self.cap, self.vgg) if e is not None and e.ema_decay > 0]

    @contextlib.contextmanager
    def ema_weights(self):
        """Inside the block the model IS its moving average: parameters and averages of every averaged store change places in place
        (vc_swap_f32: no temporary of the VGG16's size) and change back on exit, so eval_rec_loss(), a CaptionGenerator on the engine
        and everything else that reads the parameters run on the averaged weights.  Both transitions are made visible to the caches
        that key on parameter identity (CaptionEngine.param_version, the VGG16's sum-of-squares cache).  Not nestable; no training step
        inside."""
        if not self.ema_decay > 0:
            raise RuntimeError("ema_weights() needs weight averaging: give --ema_decay D (Parameters.ema_decay in (0, 1)); it is 0 = off")
        if self._ema_swapped:
            raise RuntimeError("ema_weights() is already entered: the parameters are the averages now (it does not nest)")
        w2 = self.vgg.w2_valid if self.vgg is not None else False
        self._swap_averages()
        self._ema_swapped = True
        try:
            yield self
        finally:
            self._swap_averages()
            self._ema_swapped = False
            if self.vgg is not None:
                self.vgg.w2_valid = w2   # the parameters are bit for bit the ones those sums were taken of

    def _swap_averages(self):
        st = _stream()
        self.cap.join_off_chain()
        for eng in self._ema_engines():
            S = eng.store
            self.lib.vc_swap_f32(st, P(S.p), P(S.slot("ema")), S.n)
        self.cap.param_updates += 1   # the kernel writes behind torch's back (CaptionEngine.param_version)
        if self.vgg is not None:
            self.vgg.w2_valid = False

    def load_state_dict(self, d, imagenet_path=None):
        avg = split_averages(d)
        if avg and not self.ema_decay > 0:
            print("checkpoint carries %d averaged variables (<name>%s): ignored, and not written again, with --ema_decay at its default"
                  % (len(avg), EMA_SUFFIX))
            d = {k: v for k, v in d.items() if not k.endswith(EMA_SUFFIX)}
        self._load_state_dict(d, imagenet_path)
        if self.ema_decay > 0:
            warm = [e.ema_warmup for e in self._ema_engines()]
            if all(warm):
                print("weight averaging: no <name>%s among the loaded variables: the averages start from the parameters, decay "
                      "min(%g, (1 + t) / (10 + t)) (warm-up on)" % (EMA_SUFFIX, self.ema_decay))
            else:
                print("weight averaging: averages loaded%s: constant decay %g (no warm-up: the step counter restarts at 0)"
                      % ("" if not any(warm) else " for the caption side, the cnn/* averages start from the parameters with the warm-up",
                         self.ema_decay))

    def _load_state_dict(self, d, imagenet_path):
        self.cap.load_params(d)
        cnn = {k: v for k, v in d.items() if k.startswith("cnn/") and not k.endswith(EMA_SUFFIX)}
        if self.vgg is not None:
            if not cnn and imagenet_path and os.path.exists(imagenet_path):
                # a checkpoint written without cnn/* (older runs of this build with precomputed features)
                print("checkpoint has no cnn/* variables: loading VGG16 from %s" % imagenet_path)
                self.vgg.load_weights(imagenet_path)
            else:
                self.vgg.load_params(d)
        elif cnn:
            self.cnn_host = cnn  # carried along so that the next save writes them again

    def save(self, path):
        """saver.save (main.py:286-288): the trainable variables under the reference's names
        (main.py:186-191; optimiser slots and global_step are not in its var list, Q11).
        `path` ending in .npz -> a name-keyed numpy archive; anything else is a TensorFlow V2 checkpoint
        prefix (<path>.index + <path>.data-00000-of-00001 + `checkpoint`, tf_bundle.py)."""
        if path.endswith(".npz"):
            np.savez(path, **self.state_dict())
        else:
            from . import tf_bundle
            tf_bundle.write_bundle(path, self.state_dict())

    def restore(self, path, use_ema=False):
        """saver.restore (main.py:201-204, gen_caption.py:113-115): every variable of this model must be present.
        use_ema: load each <name>/ExponentialMovingAverage of the checkpoint AS <name> (what tf.train.ExponentialMovingAverage's
        variables_to_restore() does): the model is then the averaged one for every consumer."""
        inet = getattr(self.p, "image_net_weights_path", None)
        if path.endswith(".npz"):
            with np.load(path) as z:
                d = {k: z[k] for k in z.files}
        else:
            from . import tf_bundle
            d = tf_bundle.read_bundle(path)
        if use_ema:
            avg = split_averages(d)
            if not avg:
                raise KeyError("--use_ema: checkpoint %s holds no averaged weights (<name>%s): it was written without --ema_decay"
                               % (path, EMA_SUFFIX))
            d = {k: v for k, v in d.items() if not k.endswith(EMA_SUFFIX)}
            d.update(avg)
            print("restoring the averaged weights of %d variables (--use_ema)" % len(avg))
        self.load_state_dict(d, imagenet_path=inet)
