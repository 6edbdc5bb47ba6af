#!/usr/bin/env python3
"""Phase stamps of the accumulate pass of shift_and_add (k_saa_tile<ACC>, diagnostic build -DSRX_STAMPS): C2, thread 0 of every block."""
import ctypes, os, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "enph459-super-resolution_amd"))
import torch
import sr_mi355x as S
from sr_mi355x import _lib, synth
B = int(os.environ.get("STAMPS_B", "1024"))
lr = torch.round(torch.rand((B, 16, 64, 64), device="cuda") * 255)
S.shift_and_add_batched(lr, synth.phase_shifts(4), 4)
buf = np.zeros((5, 8, 40000), dtype=np.uint64)
lib = _lib.load(); lib.srx_debug_stamps.argtypes = [ctypes.c_void_p]
assert lib.srx_debug_stamps(buf.ctypes.data_as(ctypes.c_void_p)) == 0
t = buf[2].astype(np.int64)
nb = 9 * B
# stamps 2 -> 3 hold a column pass only where frame 0 closes its group (a group of one); the first group's column pass is between stamps 6 and 7
names = ["geometry + frame 0 fetch + stash", "frame 0 row pass (+ barrier)", "frame 0 column pass (if it ends a group)", "frame 0 stash next (+ barrier)", "frames 1..N-1"]
if os.environ.get("STAMPS_STAGED"):  # the staged form (k_saa_tile<float, 4, true, G > 1>): the stamps are per chunk and group, not per frame
    names = ["geometry + first chunk staged", "first group: row passes of its chunks (+ barrier)", "first group: column pass", "first group: turn (rest of the next chunk, barrier)",
             "groups 1.."]
ok = (t[0, :nb] > 0) & (t[5, :nb] > t[0, :nb])
tot = (t[5, :nb] - t[0, :nb])[ok]
print(f"blocks {ok.sum()}, median cycles/block {np.median(tot):.0f} (p10 {np.percentile(tot, 10):.0f}, p90 {np.percentile(tot, 90):.0f})")
for i in range(5):
    d = (t[i + 1, :nb] - t[i, :nb])[ok]
    print(f"    {names[i]:42s} median {np.median(d):8.0f}  mean {d.mean():8.0f}  share {100 * d.mean() / tot.mean():5.1f} %")
print(f"    {'per frame (stamps 1 -> 5, / 16)':42s} median {np.median((t[5, :nb] - t[1, :nb])[ok]) / 16:8.0f}")
ok67 = ok & (t[6, :nb] > 0) & (t[7, :nb] > t[6, :nb])
if ok67.any():
    d = (t[7, :nb] - t[6, :nb])[ok67]
    print(f"    {'column pass of the first group':42s} median {np.median(d):8.0f}  mean {d.mean():8.0f}  share {100 * d.mean() / tot.mean():5.1f} % (one of 4)")
