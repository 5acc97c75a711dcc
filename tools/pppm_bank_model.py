#!/usr/bin/env python3
"""LDS bank model of k_pppm_force<true, *> (md_pppm.hip): the mean LDS cycles of a wave's ds_read_b64 for a mesh, a staging layout
(row stride, plane stride, in doubles) and a lane -> atom mapping.  numpy only: no GPU, no oracle.

The rule (MI355X LDS, 64 banks of 4 bytes): a wave's ds_read_b64 is served as two groups of 32 lanes; a double at index i lies on the
bank pair i mod 32; lanes of a group that read the same address are served by one access (broadcast); a group takes one cycle per
distinct address on its busiest bank pair.  A conflict-free read of a full wave therefore costs 2.0.  The offsets of the three fields
move every lane of an instruction alike and do not enter.

The kernel's reads: thread t of a 256-thread workgroup serves atoms a0 + t, a0 + t + 256, ... of its atom range, and every range starts
at a multiple of 256, so the 32 lanes of a group hold the atoms 32 g .. 32 g + 31 of the file order (`order` re-maps them).  Each charged
atom reads the 125 points (gz[c], gy[b], gx[k]) of its stencil, the same (c, b, k) in every lane of an instruction; uncharged atoms
take no part.

    python tools/pppm_bank_model.py                      PE-10k, 0.15 A jitter: the dense layout, the rule's, and a scan of plane strides
"""
import argparse
import os
import sys

import numpy as np

ORDER = 5
BANKS = 32   # bank pairs: a double's index mod 32


def lamda(d):
    """positions as fractions of the box, wrapped to [0, 1] as the kernels do (pos_lamda)"""
    b = np.asarray(d["box"], float)
    lat = np.array([[b[3] - b[0], 0, 0], [b[6], b[4] - b[1], 0], [b[7], b[8], b[5] - b[2]]])
    lam = (np.asarray(d["x"], float) - b[:3]) @ np.linalg.inv(lat)
    return lam - np.floor(lam)


def stencil(lam, n):
    """(natoms, 5) periodic grid indices i-2 .. i+2 around the nearest point of lam * n (pppm_nearest, pppm_wrap)"""
    i = np.floor(lam * n + 0.5).astype(np.int64)
    return (i[:, None] + np.arange(ORDER)[None, :] - 2) % n


def cycles_per_wave_read(grid, strides, lam, charged=None, order=None):
    """mean cycles per wave ds_read_b64 of the interpolation loop.
    grid (nx, ny, nz); strides (row stride, plane stride) in doubles; lam (natoms, 3) in [0, 1]; charged: mask of the atoms that read
    (default: all); order: lane -> atom mapping, atom order[j] sits in slot j (default: file order)."""
    nx, ny, nz = (int(v) for v in grid)
    rs, ps = int(strides[0]), int(strides[1])
    lam = np.asarray(lam, float)
    n = len(lam)
    charged = np.ones(n, bool) if charged is None else np.asarray(charged, bool)
    if order is not None:
        lam, charged = lam[np.asarray(order)], charged[np.asarray(order)]
    gx, gy, gz = stencil(lam[:, 0], nx), stencil(lam[:, 1], ny), stencil(lam[:, 2], nz)
    # addresses of the 125 reads per atom, (n, 125), in the kernel's loop order c (z), b (y), k (x)
    addr = (gz[:, :, None, None] * ps + gy[:, None, :, None] * rs + gx[:, None, None, :]).reshape(n, ORDER ** 3)
    ngroups = (n + 31) // 32
    pad = ngroups * 32 - n
    addr = np.vstack([addr, np.zeros((pad, ORDER ** 3), np.int64)]).reshape(ngroups, 32, ORDER ** 3)
    active = np.concatenate([charged, np.zeros(pad, bool)]).reshape(ngroups, 32)
    total = 0
    for g in range(ngroups):
        a = addr[g][active[g]]                      # (lanes, 125)
        if a.size == 0:
            continue
        a = np.sort(a, axis=0)                      # distinct addresses per instruction: sort the lanes, keep the first of each run
        first = np.ones_like(a, bool)
        first[1:] = a[1:] != a[:-1]
        bank = a % BANKS
        worst = np.zeros(a.shape[1], np.int64)
        for bnk in range(BANKS):
            worst = np.maximum(worst, (first & (bank == bnk)).sum(0))
        total += int(worst.sum())
    waves = (n + 63) // 64
    return total / (waves * ORDER ** 3)


def pe10k_jitter(jitter=0.15, seed=1234):
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from scema_amd.systems import build_pe
    return build_pe(6, 9, 16, jitter=jitter, seed=seed)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--grid", type=int, nargs=3, default=[12, 12, 12])
    ap.add_argument("--strides", type=int, nargs=2, default=None, metavar=("ROW", "PLANE"), help="one layout instead of the scan")
    ap.add_argument("--jitter", type=float, default=0.15)
    ap.add_argument("--seed", type=int, default=1234)
    a = ap.parse_args()
    d = pe10k_jitter(a.jitter, a.seed)
    lam, q = lamda(d), np.asarray(d["charge"]) != 0.0
    nx, ny, nz = a.grid
    if a.strides:
        print(f"{tuple(a.grid)} strides {tuple(a.strides)}: {cycles_per_wave_read(a.grid, a.strides, lam, q):.2f} cycles per wave read")
        return
    print(f"PE-10k, {a.jitter} A jitter, seed {a.seed}, mesh {nx} x {ny} x {nz}, file order; conflict-free = 2.00")
    for ps in range(nx * ny, nx * ny + 33):
        print(f"  ({nx}, {ps})  {24 * ps * nz / 1024:5.1f} KB  {cycles_per_wave_read(a.grid, (nx, ps), lam, q):5.2f}")
    for rs in (nx + 1,):
        for ps in range(rs * ny, rs * ny + 8):
            print(f"  ({rs}, {ps})  {24 * ps * nz / 1024:5.1f} KB  {cycles_per_wave_read(a.grid, (rs, ps), lam, q):5.2f}")


if __name__ == "__main__":
    main()
