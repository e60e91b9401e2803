"""Diagnostic: the launch sequence of the HIP backward, as JSON — every entry of libgroupnet_hip.so a backward calls,
with its non-address scalar arguments and, per element of a descriptor array, the non-address fields (a GEMM problem's
shape, strides, flags, alpha and beta); of an address only whether it is NULL.  Also every `torch.zeros` fill (shape).

    python tools/diag/backward_launches.py --json launches.json [--grads grads.pt --repeats 5]

The cases sit on the boundaries of `route.backward_round_route` (tests/test_backward_route_gpu.py) plus the
`MultiScaleHGNN([2, 5, 11])` training step at B = 8, N = 11.  Two trees that print the same JSON launch the same backward.
--grads: the forward outputs, d h and every parameter gradient of each case and repeat, for comparing two trees."""
import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import torch

from groupnet_amd import MS_HGNN_batch as M, _lib, backward, ops
from groupnet_amd.multiscale import MultiScaleHGNN
from test_backward_gpu import _modules

dev = torch.device("cuda:0")
BOTH, FACTORS = (True, True), (False, True)
CASES = {       # B, N, nmp_layers, (module, which of (node_feat, factors) the loss reads)
    "pair+hyper": (2, 5, 1, (("pair", BOTH), ("hyper", BOTH))),
    "pair+hyper-nmp2": (2, 5, 2, (("pair", BOTH), ("hyper", BOTH))),
    "live-subset": (2, 5, 1, (("pair", FACTORS), ("hyper", BOTH))),
    "pair-largest-scene": (1, 140, 1, (("pair", BOTH),)),
    "pair-first-beyond": (1, 141, 1, (("pair", BOTH),)),
    "hyper-beyond": (1, 141, 1, (("hyper", BOTH),)),
    "pair+hyper-beyond": (1, 141, 1, (("pair", BOTH), ("hyper", BOTH))),
}


def describe(value, ctype):
    if isinstance(value, ctypes.Array) and issubclass(value._type_, ctypes.Structure):
        return [{name: describe(getattr(el, name), t) for name, t in el._fields_} for el in value]
    if ctype is _lib._P or isinstance(value, ctypes.c_void_p):
        return "null" if not (value.value if isinstance(value, ctypes.c_void_p) else value) else "address"
    if isinstance(value, (int, float)):
        return value
    return "null" if value is None else "reference"


class Recorder:
    def __init__(self):
        self.calls, self.on = [], False
        lib = _lib.load()
        for name, (_, argtypes) in _lib.SIGNATURES.items():
            setattr(lib, name, self.through(name, getattr(lib, name), argtypes))
        zeros = torch.zeros

        def zeros_through(*shape, **kw):
            if self.on and shape:
                self.calls.append(["torch.zeros", list(shape[0]) if isinstance(shape[0], (tuple, list)) else list(shape)])
            return zeros(*shape, **kw)
        torch.zeros = zeros_through

    def through(self, name, real, argtypes):
        def call(*args):
            if self.on:
                self.calls.append([name] + [describe(a, t) for a, t in zip(args, argtypes)])
            return real(*args)
        return call

    def backward(self, fn):
        self.calls, self.on = [], True
        try:
            out = fn()
            torch.cuda.synchronize()
        finally:
            self.on = False
        return out, self.calls


def run_case(rec, name):
    B, N, nmp, modules = CASES[name]
    pair, hyper = _modules(500 + N, nmp)
    mods = [(pair if kind == "pair" else hyper).to(dev).train() for kind, _ in modules]
    g = torch.Generator().manual_seed(N + nmp)
    x = torch.randn(B, N, 64, generator=g).to(dev)
    H = ops.topk_incidence(ops.affinity(x), [3])[0]
    Hs = [None if kind == "pair" else H for kind, _ in modules]
    U = [[torch.rand(B, N * N if kind == "pair" else N, m.edge_types, generator=g).to(dev) for _ in range(nmp)]
         for m, (kind, _) in zip(mods, modules)]
    traces = [backward.ModuleTrace(m, x, h) for m, h in zip(mods, Hs)]
    with torch.no_grad(), M.training_call():
        res = M.run_message_passing(mods, [x] * len(mods), Hs, U, [None] * len(mods), traces=traces)
    g_out = [[torch.randn(t.shape, generator=g).to(dev) if used else None for t, used in zip(r, outputs)]
             for r, (_, outputs) in zip(res, modules)]
    (dxs, grads), calls = rec.backward(lambda: backward.modules_backward(traces, [a for a, _ in g_out], [b for _, b in g_out]))
    tensors = {f"out{i}.{k}": t for i, r in enumerate(res) for k, t in zip(("nf", "fac"), r)}
    tensors.update({f"dx{i}": t for i, t in enumerate(dxs)})
    tensors.update({f"m{i}.{k}": grads[p] for i, m in enumerate(mods) for k, p in m.named_parameters() if p in grads})
    return calls, tensors


def run_block(rec):
    B, N = 8, 11
    torch.manual_seed(3)
    blk = MultiScaleHGNN([2, 5, 11]).to(dev).train()
    g = torch.Generator().manual_seed(4)
    f = torch.randn(B, N, 64, generator=g).to(dev).requires_grad_(True)
    noise = [[torch.rand(s, generator=g).to(dev)] for s in blk.noise_shapes(B, N)]
    out, _ = blk(f, noise_u=noise)
    loss = (out * torch.randn(out.shape, generator=g).to(dev)).sum()
    _, calls = rec.backward(loss.backward)
    tensors = {"out": out.detach(), "dx": f.grad}
    tensors.update({k: p.grad for k, p in blk.named_parameters() if p.grad is not None})
    return calls, tensors


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", required=True)
    ap.add_argument("--grads")
    ap.add_argument("--repeats", type=int, default=1)
    a = ap.parse_args()
    rec, launches, saved = Recorder(), {}, {}
    for name in list(CASES) + ["block-2-5-11"]:
        for rep in range(a.repeats):
            calls, tensors = run_block(rec) if name == "block-2-5-11" else run_case(rec, name)
            assert rep == 0 or calls == launches[name], name
            launches[name] = calls
            saved[f"{name}/{rep}"] = {k: t.detach().cpu().clone() for k, t in tensors.items()}
        print(f"{name}: {len(calls)} calls")
    with open(a.json, "w") as fh:
        json.dump(launches, fh, indent=0, sort_keys=True)
    if a.grads:
        torch.save(saved, a.grads)


if __name__ == "__main__":
    main()
