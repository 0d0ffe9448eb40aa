"""Decoding controls timing on one GPU (DESIGN.md "Decoding controls"), by the protocol of trunc_time.py.
(a) vc_decode_controls_f32 beside the launches a round already has at the same rows -- vc_decode_pick_f32 (argmax) and
    vc_decode_round_end_i32 -- on 640 rows of V = 10 000 logits: the candidate layout (histories of 15 of max_len 30 words, skip 0) and
    the beam layout (128 images x 5 beams, skip 1), with no-repeat bigrams + min_len 5 + penalty 1.2 + 8 banned words.  Each entry's
    `--launches` back-to-back launches are captured into one hipGraph; device events around a replay, the entries alternating inside a
    repetition, median over `--reps` after two warm-up repetitions; microseconds per launch.
(b) one decoder round with the controls off and on, at full dimensions (V = 10 000, decoder_hidden 512, gen_z_samples 100, latent 150,
    Normal prior, random weights): diverse(draws=20) on 32 images (640 rows, max_len 30) and beam_search(beam_size=5) on 128 images, both
    with check_every=0 so that every call runs all of its rounds; host clock around a synchronised call, off and on alternating,
    median; microseconds per round = call / rounds.  Controls off is the call without the keyword, launch for launch.
Prints one JSON line per measurement.
    python tools/experiments/controls_time.py [--reps 7] [--launches 50] [--skip-rounds]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from vae_captioning_amd import abi, spec  # noqa: E402
from vae_captioning_amd.controls import DecodeControls  # noqa: E402
from vae_captioning_amd.engine import CaptionEngine  # noqa: E402
from vae_captioning_amd.generate import CaptionGenerator  # noqa: E402
from vae_captioning_amd.utils.parameters import Parameters  # noqa: E402

P = abi.ptr
BANNED = [11, 12, 13, 14, 15, 16, 17, 18]
CONTROLS = dict(no_repeat_ngram=2, min_len=5, repetition_penalty=1.2, banned=BANNED)


def kernel_times(lib, R, V, Lmax, reps, launches):
    st = torch.cuda.current_stream().cuda_stream
    g = torch.Generator(device="cuda").manual_seed(R)
    x = torch.randn((R, V), device="cuda", generator=g) * 4.0
    i32 = dict(dtype=torch.int32, device="cuda")
    hist = torch.randint(3, 60, (R, Lmax), generator=g, device="cuda").to(torch.int32)   # (a small alphabet: repeats are common)
    ln = torch.full((R,), Lmax // 2, **i32)
    tok, done, seq, ln2 = (torch.zeros(R, **i32) for _ in range(4))
    lp, pending = torch.zeros(R, dtype=torch.float64, device="cuda"), torch.zeros(1, device="cuda")
    table = torch.tensor(BANNED, **i32)

    def controls(skip):
        return lambda: lib.vc_decode_controls_f32(st, P(x), R, V, V, P(hist), Lmax, Lmax, skip, P(ln), None, 2, 5, 2, 1.2, P(table), len(BANNED))

    fns = [("vc_decode_pick_f32 (argmax)", lambda: lib.vc_decode_pick_f32(st, P(x), R, V, V, 1.0, None, 1, None, -1, P(tok), P(done), P(seq), 1,
                                                                          P(ln2), P(lp))),
           ("vc_decode_round_end_i32", lambda: lib.vc_decode_round_end_i32(st, P(done), R, P(pending), None)),
           ("vc_decode_controls_f32 skip 0", controls(0)), ("vc_decode_controls_f32 skip 1", controls(1))]
    ts, graphs = {name: [] for name, _ in fns}, {}
    for name, fn in fns:
        fn()   # (eager once: the code object is loaded before the capture)
        torch.cuda.synchronize()
        graphs[name] = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graphs[name]):
            st = torch.cuda.current_stream().cuda_stream
            for _ in range(launches):
                fn()
    st = torch.cuda.current_stream().cuda_stream
    for rep in range(reps + 2):   # (two warm-up repetitions)
        for name, _ in fns:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            graphs[name].replay()
            e1.record()
            torch.cuda.synchronize()
            if rep >= 2:
                ts[name].append(e0.elapsed_time(e1) * 1e3 / launches)
    for name, _ in fns:
        print(json.dumps({"rows": R, "V": V, "Lmax": Lmax, "entry": name, "us_per_launch": round(float(np.median(ts[name])), 2),
                          "min_us": round(min(ts[name]), 2), "max_us": round(max(ts[name]), 2)}))


def round_times(lib, reps):
    p = Parameters()
    p.mode, p.num_captions, p.prior = "inference", 1, "Normal"
    V = 10000
    eng = CaptionEngine(p, V, lib=lib)
    eng.load_params(spec.init_caption_params(p, V, seed=3))
    gen = CaptionGenerator(eng)
    rng = np.random.default_rng(0)
    feats = np.maximum(rng.standard_normal((128, p.cnn_feature_size)), 0).astype(np.float32)
    ctl = DecodeControls(**CONTROLS)
    T = p.gen_max_len
    settings = [("diverse 32 images x 20 draws (640 rows)", T, lambda **kw: gen.diverse(feats[:32], draws=20, max_len=T, check_every=0, **kw)),
                ("beam_search 128 images x 5 beams (640 rows)", T - 1, lambda **kw: gen.beam_search(feats, beam_size=5, max_len=T, check_every=0, **kw))]
    for name, rounds, call in settings:
        ts = {"off": [], "on": []}
        for rep in range(reps + 2):
            for which, kw in (("off", {}), ("on", dict(controls=ctl))):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                call(**kw)
                torch.cuda.synchronize()
                if rep >= 2:
                    ts[which].append((time.perf_counter() - t0) * 1e3)
        off, on = float(np.median(ts["off"])), float(np.median(ts["on"]))
        print(json.dumps({"setting": name, "rounds": rounds, "call_ms_off": round(off, 3), "call_ms_on": round(on, 3),
                          "min_ms_off": round(min(ts["off"]), 3), "max_ms_off": round(max(ts["off"]), 3), "min_ms_on": round(min(ts["on"]), 3),
                          "max_ms_on": round(max(ts["on"]), 3), "us_per_round_off": round(off * 1e3 / rounds, 1),
                          "us_per_round_on": round(on * 1e3 / rounds, 1), "added_us_per_round": round((on - off) * 1e3 / rounds, 1)}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--skip-rounds", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("controls_time.py measures on a GPU: none found")
    lib = abi.load()
    kernel_times(lib, 640, 10000, 30, a.reps, a.launches)
    if not a.skip_rounds:
        round_times(lib, a.reps)


if __name__ == "__main__":
    main()
