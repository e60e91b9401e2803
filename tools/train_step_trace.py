#!/usr/bin/env python3
"""Eager training steps of the config-4 block in fp32 for a kernel trace: MultiScaleHGNN([2, 4, 8, 16]) at B = 1024,
N = 50, device noise, in the dense or the bit-mask incidence form.

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python3 tools/train_step_trace.py mask [steps]

Every step is the same launches, so a kernel's total over the trace / steps is its share of one step."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))   # repo root
import groupnet_amd as G
from groupnet_amd import ops
from groupnet_amd.multiscale import MultiScaleHGNN

form = sys.argv[1] if len(sys.argv) > 1 else "dense"
steps = int(sys.argv[2]) if len(sys.argv) > 2 else 3
ops.set_incidence_form(form)
dev = torch.device("cuda:0")
torch.manual_seed(0)
B, N = 1024, 50
blk = MultiScaleHGNN([2, 4, 8, 16]).to(dev).train()
f = torch.randn(B, N, 64, device=dev)
tgt = torch.randn(B, N, blk.out_features, device=dev)
opt = torch.optim.SGD(blk.parameters(), lr=1e-3)
G.set_noise_mode("device", seed=1, offset=0)
try:
    for _ in range(steps):
        opt.zero_grad()
        out, _ = blk(f)
        loss = ((out - tgt) ** 2).mean()
        loss.backward()
        opt.step()
    torch.cuda.synchronize()
finally:
    G.set_noise_mode("host")
print(f"{form}: {steps} eager training steps at B={B}, N={N}, loss {float(loss):.6f}")
