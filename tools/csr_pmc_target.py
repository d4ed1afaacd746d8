"""Target of the rocprofv3 runs over the fused CSR kernels (profiles/csr/): every forest of tools/csr_time.py that has a fused
form, its tile strategy forced, 200 k rows with 5 % of the entries stored, three predict_csr calls each.
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/csr_pmc_target.py
    rocprofv3 --pmc <counters> -d <dir> -- python tools/csr_pmc_target.py         (a run of its own)"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import csr_time  # noqa: E402

for name, cols, tile, make in csr_time.forests():
    if tile is None:
        continue
    f = make()
    f.set_strategy(getattr(csr_time.ta, "STRATEGY_" + tile))
    x, ip, ix, vals = csr_time.make_rows(cols, 0.05, seed=50 + cols)
    for _ in range(3):
        out = f.predict_csr(ip, ix, vals)
    torch.cuda.synchronize()
    f.check()
    f.close()
