"""SHA-256 of everything mpe_mlp_grad and mpe_mlp_dinput write at the ABI on the small cases of their tests: a tool for before /
after a change to the two backward kernels (csrc/mpe_mlp_grad.hip, csrc/mpe_mlp_dinput.hip, csrc/mpe_mlp_device.h).

    MPE_HIP_LIB=<libmpe_hip.so> python tools/mlp_back_bits.py [--out FILE]      one JSON object {name: digest}

mpe_mlp_grad: every case of tests/_mlp_grad_ref.GPU_CASES and WALK_EXTRA, inputs from make_inputs -- the packed gradient and the
workspace, each whole with the sentinels around it.  mpe_mlp_dinput: every (case, window) of tests/_mlp_dinput_ref.runs() and
WALK_EXTRA's whole row, on the 16-byte and on the 4-byte store path -- every agent's din buffer, whole, sentinels included.  MPE_HIP_LIB
picks the library (_abi.py), so one script serves two builds on one machine; the digests depend on the compiler version: not a test."""
import argparse
import ctypes as C
import hashlib
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from multiagent_particle_envs_amd import _abi      # noqa: E402
import _mlp_grad_ref as R                          # noqa: E402
import _mlp_dinput_ref as D                        # noqa: E402

SENTINEL, PAD = -777.25, 64


def digest(*tensors):
    torch.cuda.synchronize()
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.cpu().numpy().tobytes())
    return h.hexdigest()


def rows_on_device(x, agents, shift, dev):
    """in and dout of every agent, `shift` floats into their allocations -> (the tensors, in pointers, dout pointers)"""
    held, ins, douts = [], [], []
    for i in agents:
        for src, dst in ((x["in"][i], ins), (x["dout"][i], douts)):
            flat = torch.full((src.size + shift,), SENTINEL, dtype=torch.float32, device=dev)
            flat[shift:] = torch.tensor(np.ascontiguousarray(src), device=dev).reshape(-1)
            held.append(flat)
            dst.append(flat.data_ptr() + 4 * shift)
    return held, ins, douts


def grad_bits(out, case, dev):
    x = R.make_inputs(case)
    A, total = len(case.agents), R.offsets(case)[1]
    w = torch.tensor(R.pack(case, x), device=dev)
    held, ins, douts = rows_on_device(x, range(A), 1 if case.shift else 0, dev)
    aset = R.fill_set(_abi.MpeActorSet(), case, w.data_ptr(), _abi.MPE_POLICY_VALUE if case.value else _abi.MPE_POLICY_GREEDY)
    n_work = int(_abi.lib().mpe_mlp_grad_work(C.byref(aset), case.M))
    grad = torch.full((PAD + total + PAD,), SENTINEL, dtype=torch.float32, device=dev)
    work = torch.full((PAD + n_work + PAD,), SENTINEL, dtype=torch.float32, device=dev)
    _abi.check(_abi.lib().mpe_mlp_grad(C.byref(aset), (C.c_void_p * A)(*ins), (C.c_void_p * A)(*douts), case.M, grad.data_ptr() + 4 * PAD,
                                       work.data_ptr() + 4 * PAD, _abi.raw_stream(dev)), "mpe_mlp_grad")
    out["grad.%s.packed" % case.name], out["grad.%s.work" % case.name] = digest(grad), digest(work)


def dinput_bits(out, case, kind, dev):
    x = D.make_inputs(case)
    A, M, win = len(case.agents), case.M, D.windows(case, kind)
    w = torch.tensor(D.pack(case, x), device=dev)
    aset = D.fill_set(_abi.MpeActorSet(), case, w.data_ptr(), _abi.MPE_POLICY_VALUE)
    for path, shift in (("store16", 0), ("store4", 1)):      # store4: ld = ncol + 3, every pointer 4 bytes past a 16-byte boundary
        held, ins, douts = rows_on_device(x, range(A), shift, dev)
        desc, bufs, ptrs = _abi.MpeMlpDinput(), [], []
        for i, (c0, nc) in enumerate(win):
            ld = nc + 3 * shift
            desc.col0[i], desc.ncol[i], desc.ld[i] = c0, nc, ld
            bufs.append(torch.full((PAD + shift + (M + 2) * ld + PAD,), SENTINEL, dtype=torch.float32, device=dev))
            ptrs.append(bufs[-1].data_ptr() + 4 * (PAD + shift))
        _abi.check(_abi.lib().mpe_mlp_dinput(C.byref(aset), C.byref(desc), (C.c_void_p * A)(*ins), (C.c_void_p * A)(*douts), M,
                                             (C.c_void_p * A)(*ptrs), _abi.raw_stream(dev)), "mpe_mlp_dinput")
        out["dinput.%s.%s.%s" % (case.name, kind, path)] = digest(*bufs)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "mlp_back_bits needs a GPU"
    dev = torch.device("cuda", torch.cuda.current_device())
    out = {}
    for case in R.GPU_CASES + [R.WALK_EXTRA]:
        grad_bits(out, case, dev)
    for case, kind in D.runs() + [(D.WALK_EXTRA, "whole")]:
        dinput_bits(out, case, kind, dev)
    line = json.dumps(out, sort_keys=True)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
