#!/usr/bin/env python3
"""Fingerprint of the REFERENCE's seeded default initialisation, for test_capi_cpu.py::test_same_seed_same_init_as_reference.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_init.py <reference checkout>

Imports model/MS_HGNN_batch.py of the reference checkout unmodified, seeds torch with 5, builds the pairwise and the
hyper module (nmp_layers=2) and writes, for every state_dict entry in order, its name, its shape and the SHA-256 of its
float32 bytes.  A hash pins every bit of the ~1 M initial values in a few kilobytes (the values themselves would take
3.7 MB); only data is written.
"""
import hashlib
import json
import os
import sys
import warnings

import torch

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "init_seed5_nmp2.json")
KW = dict(h_dim=64, mlp_dim=64, bottleneck_dim=64, batch_norm=0, nmp_layers=2)
MODULES = (("pairwise", "MS_HGNN_oridinary", dict(embedding_dim=16)),
           ("hyper", "MS_HGNN_hyper", dict(embedding_dim=64, scale=3)))


def fingerprint(state_dict):
    return [[k, list(v.shape), hashlib.sha256(v.detach().to(torch.float32).contiguous().numpy().tobytes()).hexdigest()]
            for k, v in state_dict.items()]


if __name__ == "__main__":
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    sys.dont_write_bytecode = True
    sys.path.insert(0, sys.argv[1])
    warnings.filterwarnings("ignore")
    from model import MS_HGNN_batch as ref  # noqa: E402
    out = {}
    for name, cls, extra in MODULES:
        torch.manual_seed(5)
        out[name] = fingerprint(getattr(ref, cls)(**extra, **KW).state_dict())
    with open(OUT, "w") as f:      # one entry per line
        f.write("{\n" + ",\n".join(f"{json.dumps(name)}: [\n" + ",\n".join(json.dumps(e) for e in entries) + "\n]"
                                   for name, entries in out.items()) + "\n}\n")
    print(OUT, {k: len(v) for k, v in out.items()})
