"""Launch-trace recorder for VggEngine (tests/test_gpu_vgg_trace.py): what the engine asks of the library and of the stream
structure during one forward + backward, in program order, without anything that depends on addresses.

Every vc_* call whose first argument is a stream becomes [entry name, stream ordinal, [arguments]]: scalars as passed, a pointer only
as 0 (null) / 1.  Stream ordering becomes ["wait_stream", waiter, waited], ["wait_event", waiter, event] and ["record", event, stream];
streams are 0 = the caller's, 1 / 2 = the engine's two side streams, events are numbered in order of first appearance.  Host-only
queries (*_supported, *_preferred, *_workspace_bytes, *_words) are passed through unrecorded."""
import contextlib

import numpy as np
import torch

from vae_captioning_amd import spec
from vae_captioning_amd.trainer import VggEngine
from vae_captioning_amd.utils.parameters import Parameters

QUERIES = ("_supported", "_preferred", "_workspace_bytes", "_words")

# case -> (batch, training, precision, one_stream, use_wino, environment)
CASES = {
    "b2_f32_three_streams": (2, True, "f32", False, True, {}),
    "b2_f32_one_stream": (2, True, "f32", True, True, {}),
    "b2_bf16x3_three_streams": (2, True, "bf16x3", False, True, {}),
    "b2_bf16x3_wgrad_bx_off": (2, True, "bf16x3", False, True, {"VC_WGRAD_BX": "0"}),
    "b1_f32": (1, True, "f32", False, True, {}),
    "b2_not_training": (2, False, "f32", False, True, {}),
    "b1_no_wino": (1, True, "f32", False, False, {}),
}


class RecordingLib(object):
    """Stands in for abi.Lib: forwards every attribute, appends the launches to `log` while `on`."""

    def __init__(self, lib, log, stream_ordinal):
        self._lib, self._log, self._ord, self.on = lib, log, stream_ordinal, False
        self._protos = lib._protos

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        args = self._protos.get(name, (None, []))[1] if name.startswith("vc_") else []
        if not args or args[0] != ("void*", "stream") or name.endswith(QUERIES):
            return fn
        is_ptr = [t.endswith("*") for t, _ in args]

        def call(*a):
            if self.on:
                assert len(a) == len(args), name
                self._log.append([name, self._ord(a[0]), [int(v is not None and v != 0) if p else v for v, p in zip(a[1:], is_ptr[1:])]])
            return fn(*a)
        return call


@contextlib.contextmanager
def recording(eng, log):
    """Route eng's library calls and torch's stream-ordering calls into `log` while the caller holds rec.on True."""
    handles = {torch.cuda.current_stream().cuda_stream: 0}
    for i, s in ((1, eng._side), (2, eng._side2)):
        if s is not None:
            handles[s.cuda_stream] = i
    events = {}
    ordinal = lambda h: handles[int(h or 0)]
    so = lambda s: ordinal(s.cuda_stream)
    ev = lambda e: events.setdefault(id(e), len(events))
    rec = RecordingLib(eng.lib, log, ordinal)
    keep = []   # (events stay alive while their id() is a key)
    orig = (torch.cuda.Stream.wait_stream, torch.cuda.Stream.wait_event, torch.cuda.Event.record)

    def wait_stream(self, other):
        on = rec.on
        if on:
            log.append(["wait_stream", so(self), so(other)])
        rec.on = False   # (torch may build wait_stream from an event of its own: not the engine's structure)
        try:
            return orig[0](self, other)
        finally:
            rec.on = on

    def wait_event(self, event):
        if rec.on:
            keep.append(event)
            log.append(["wait_event", so(self), ev(event)])
        return orig[1](self, event)

    def record(self, stream=None):
        if rec.on:
            keep.append(self)
            log.append(["record", ev(self), so(stream if stream is not None else torch.cuda.current_stream())])
        return orig[2](self) if stream is None else orig[2](self, stream)

    real, eng.lib = eng.lib, rec
    torch.cuda.Stream.wait_stream, torch.cuda.Stream.wait_event, torch.cuda.Event.record = wait_stream, wait_event, record
    try:
        yield rec
    finally:
        torch.cuda.Stream.wait_stream, torch.cuda.Stream.wait_event, torch.cuda.Event.record = orig
        eng.lib = real


def trace_case(lib, case, setenv):
    """The launch trace of the SECOND of two forward + backward steps of `case` (the first one allocates: its zero-fill waits are
    not part of the steady state).  setenv(name, value) sets an environment variable for the duration of the caller's test."""
    B, training, precision, one_stream, use_wino, env = CASES[case]
    for k, v in env.items():
        setenv(k, v)
    p = Parameters()
    p.fine_tune = True
    p.mode = "training" if training else "inference"
    rng = np.random.default_rng(5)
    eng = VggEngine(p, lib=lib)
    eng.precision, eng.one_stream, eng.use_wino = precision, one_stream, use_wino
    eng.load_params(spec.init_vgg_params(seed=3))
    ones = np.ones((B, 4096), np.float32)
    eng.set_masks(ones, ones)
    img = torch.from_numpy(rng.integers(0, 256, size=(B, 224, 224, 3)).astype(np.float32)).cuda()
    dfc2 = torch.from_numpy(rng.normal(size=(B, 4096)).astype(np.float32)).cuda()
    log = []
    with recording(eng, log) as rec:
        for step in range(2):
            rec.on = step == 1
            eng.forward(img)
            eng.backward(dfc2)
    torch.cuda.synchronize()
    return log
