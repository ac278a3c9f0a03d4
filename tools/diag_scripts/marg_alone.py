import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import torch
from _gfbe_import import gf
abi, synth = gf.abi, gf.synth
scns = [synth.Scenario(seed=20250708 + 2 + 100 * u, n_landmarks=2000, use_wheel=True) for u in range(8)]
be = gf.Backend(0)
firsts = be.solve_batch([s.window(0) for s in scns], abi.MARGIN_OLD)
snaps = [s.window(1, state=synth.shift_state_for_next_window(s, r["state"], 1), prior=r["prior"]) for s, r in zip(scns, firsts)]
b = be.batch_upload([snaps[i % 8] for i in range(512)])
b.solve(abi.MARGIN_OLD); torch.cuda.synchronize()
be.profile_enable(True)      # (kernels one after the other)
for _ in range(3): b.solve(abi.MARGIN_OLD)
torch.cuda.synchronize()
