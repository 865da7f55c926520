"""Time `mpe_render` (MultiAgentEnv.render(mode='rgb_array'), csrc/mpe_render.hip) with device events and print one JSON line:
per config the microseconds per call and the written bytes per second, against 8 TB/s (the MI355X's HBM peak).

    python tools/render_rate.py [--iters 200] [--warmup 20] [--out FILE]

Configs (simple_spread at the reference's shared viewer, worlds at their device reset positions):
    4096 worlds at 84 x 84     (86.7 MB per call: pixel observations for a training batch)
    64 worlds at 700 x 700     (94.1 MB per call: the reference's frame size, video logging across a batch)
    simple_spread N = 64, 256 worlds at 128 x 128   (128 entities: the culling path under load)
The written bytes are V * K * size * size * 3 (the output, written once); the kernel reads a few KB of state besides.
Run it under `rocprofv3 --kernel-trace --stats` for the kernel time alone (k_render)."""
import argparse
import ctypes as C
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

import multiagent_particle_envs_amd as mpe  # noqa: E402
from multiagent_particle_envs_amd import _abi  # noqa: E402

PEAK = 8.0e12
CONFIGS = [("spread3_4096x84", "simple_spread", {}, 4096, 84),
           ("spread3_64x700", "simple_spread", {}, 64, 700),
           ("spread64_256x128", "simple_spread", {"num_agents": 64}, 256, 128)]


def time_config(name, scenario, kw, B, size, iters, warmup):
    env = mpe.make_env(scenario, batch_size=B, **kw)
    env.reset()
    desc, args, out, keep = env._render_args(None, size)
    L, stream = _abi.lib(), env._stream()
    for _ in range(warmup):
        _abi.check(L.mpe_render(C.byref(desc), C.byref(args), stream), "mpe_render")
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(iters):
        L.mpe_render(C.byref(desc), C.byref(args), stream)
    t1.record()
    torch.cuda.synchronize()
    us = t0.elapsed_time(t1) * 1e3 / iters
    nbytes = out.numel()
    drawn = float((out != 255).any(dim=-1).float().mean())
    return {"config": name, "worlds": B, "size": size, "entities": len(env.world.entities), "bytes_written": nbytes,
            "us_per_call": round(us, 2), "GBps": round(nbytes / us * 1e-3, 1), "frac_of_8TBps": round(nbytes / (us * 1e-6) / PEAK, 3),
            "drawn_pixel_fraction": round(drawn, 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("render_rate.py times the kernel on a GPU: no device visible")
    rows = [time_config(*c, a.iters, a.warmup) for c in CONFIGS]
    line = json.dumps({"tool": "render_rate", "device": torch.cuda.get_device_name(0), "iters": a.iters, "configs": rows})
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
