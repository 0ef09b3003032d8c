#!/usr/bin/env python3
"""torch's CPU bfloat16 + and * on the pair sets of _half_ref ("bfloat16":
exhaustive_pairs and product_pairs), saved as bit patterns for
tests/test_half_ref.py: arrays "<set>_sum" and "<set>_prod".

usage: _half_torch_native.py OUT.npz

A process of its own: torch's wheel carries a HIP runtime, and the pytest
process may already hold the library's (one process, one runtime).
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _half_ref as R  # noqa: E402

out = {}
for name, pairs in R.PAIR_SETS.items():
    a, b = pairs("bfloat16")
    x = torch.from_numpy(a.view(np.int16)).view(torch.bfloat16)
    y = torch.from_numpy(b.view(np.int16)).view(torch.bfloat16)
    out[f"{name}_sum"] = (x + y).view(torch.int16).numpy().view(np.uint16)
    out[f"{name}_prod"] = (x * y).view(torch.int16).numpy().view(np.uint16)
np.savez(sys.argv[1], **out)
