#!/usr/bin/env python3
"""torch's CPU bfloat16 + and * on _half_ref.exhaustive_pairs("bfloat16"), saved
as bit patterns for tests/test_half_ref.py.

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

a, b = R.exhaustive_pairs("bfloat16")
x = torch.from_numpy(a.view(np.int16)).view(torch.bfloat16)
y = torch.from_numpy(b.view(np.int16)).view(torch.bfloat16)
np.savez(sys.argv[1], sum=(x + y).view(torch.int16).numpy().view(np.uint16),
         prod=(x * y).view(torch.int16).numpy().view(np.uint16))
