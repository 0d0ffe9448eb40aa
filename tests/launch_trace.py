"""Launch-trace recorder (tests/test_gpu_vgg_trace.py, tests/test_gpu_decode_trace.py): what an engine or a generator asks of the library,
of the stream structure and of its captured graphs, in program order, without anything that depends on addresses.

Every vc_* call whose first argument is a stream becomes [entry name, stream ordinal, [arguments]]: scalars as passed, a pointer only
as 0 (null) / 1.  Stream ordering becomes ["wait_stream", waiter, waited], ["wait_event", waiter, event] and ["record", event, stream];
graphs become ["capture_begin"], ["capture_end"] and ["replay", graph].  Stream ordinals come from the map the caller gives (VggEngine:
0 = the caller's, 1 / 2 = the engine's two side streams); a stream outside it, and every event and graph, is numbered in order of first
appearance (a graph appears when its capture begins).  Host-only queries (*_supported, *_preferred, *_workspace_bytes, *_words) are
passed through unrecorded."""
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
def recording(objs, log, streams=None):
    """Route the library calls of `objs` (everything whose .lib to swap: an engine, its generator) and torch's stream-ordering and
    graph calls into `log` while the caller holds rec.on True.  streams: {stream handle: ordinal} of the streams known beforehand."""
    handles = dict(streams if streams is not None else {torch.cuda.current_stream().cuda_stream: 0})
    events, graphs = {}, {}

    def ordinal(h):
        h = int(h or 0)
        if h not in handles:
            handles[h] = max(handles.values(), default=-1) + 1
        return handles[h]

    so = lambda s: ordinal(s.cuda_stream)
    keep = []   # (events and graphs stay alive while their id() is a key)

    def number(table, obj):
        if id(obj) not in table:
            keep.append(obj)
            table[id(obj)] = len(table)
        return table[id(obj)]

    rec = RecordingLib(objs[0].lib, log, ordinal)
    Graph = torch.cuda.CUDAGraph
    orig = (torch.cuda.Stream.wait_stream, torch.cuda.Stream.wait_event, torch.cuda.Event.record)
    orig_graph = (Graph.capture_begin, Graph.capture_end, Graph.replay)

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
            log.append(["wait_event", so(self), number(events, event)])
        return orig[1](self, event)

    def record(self, stream=None):
        if rec.on:
            log.append(["record", number(events, self), so(stream if stream is not None else torch.cuda.current_stream())])
        return orig[2](self) if stream is None else orig[2](self, stream)

    def capture_begin(self, *a, **k):
        if rec.on:
            number(graphs, self)
            log.append(["capture_begin"])
        return orig_graph[0](self, *a, **k)

    def capture_end(self):
        if rec.on:
            log.append(["capture_end"])
        return orig_graph[1](self)

    def replay(self):
        if rec.on:
            log.append(["replay", number(graphs, self)])
        return orig_graph[2](self)

    real = [o.lib for o in objs]
    assert all(r is real[0] for r in real)
    for o in objs:
        o.lib = rec
    torch.cuda.Stream.wait_stream, torch.cuda.Stream.wait_event, torch.cuda.Event.record = wait_stream, wait_event, record
    Graph.capture_begin, Graph.capture_end, Graph.replay = capture_begin, capture_end, replay
    try:
        yield rec
    finally:
        torch.cuda.Stream.wait_stream, torch.cuda.Stream.wait_event, torch.cuda.Event.record = orig
        Graph.capture_begin, Graph.capture_end, Graph.replay = orig_graph
        for o, r in zip(objs, real):
            o.lib = r


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
    streams = {torch.cuda.current_stream().cuda_stream: 0}
    for i, s in ((1, eng._side), (2, eng._side2)):
        if s is not None:
            streams[s.cuda_stream] = i
    with recording([eng], log, streams) as rec:
        for step in range(2):
            rec.on = step == 1
            eng.forward(img)
            eng.backward(dfc2)
    torch.cuda.synchronize()
    return log
