"""Exact-data cases for the three k-means Lloyd-pass kernels (csrc/kernels/cluster.hip), shared by
tests/test_kmeans_kernels.py and by the per-mode child process it starts (``python
_kmeans_cases.py``: the arithmetic knobs AVMI_KMEANS_* are read once per process).

Every check returns a list of failure strings (empty = passed), so the child can report all of them
in its one-line JSON verdict and the tests can ``assert not failures``.

A. integer battery: X and C hold integers in [-4, 4].  Every product, score, ||c||^2 / 2,
   workgroup partial sum and ||x||^2 is then an integer or half-integer far below 2^24, exact in
   fp32, and every value is exact in ONE bf16 term, so each kernel in each mode must reproduce the
   int64 reference bit for bit, including the lowest-index rule on the (frequent) exact ties.
C. fp32-exact partial sums: 20-bit coordinates in [1, 2) (x 2^13), <= 16 rows per cluster and
   workgroup, so every workgroup sum fits 24 bits and is exact in fp32 in any order.
"""
from __future__ import annotations

import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402

# (D, k) by dispatch arm of km_variant
SCORE_SHAPES = [(4, 3), (4, 16), (4, 17), (8, 20), (8, 32), (16, 1), (16, 15), (16, 16), (16, 31), (32, 7),
                (32, 16)]
MFMA_SHAPES = [(2, 3), (64, 5), (16, 40), (32, 100)]
LDS_SHAPES = [(16, 300), (64, 70)]
MULTI_RUNS = [(16, [1, 3, 16, 7]), (4, list(range(1, 17)))]          # (D, ks): MFMA kernel, R = 4 / 16
SMALL_N = (1, 63, 64, 65, 257)
# every wave runs >= 3 tiles of 64 rows with a ragged tail on a grid of 256 workgroups of 4 waves
BIG_N = 64 * (3 * 1024 + 37) + 17
TIE_N = 257             # smallest row count at which the tie share is asserted
MIN_TIE_SHARE = 0.05


def tie_run(ks) -> int:
    return max(range(len(ks)), key=lambda r: ks[r])


def int_data(n: int, D: int, ks: list[int], seed: int, dup: bool = False):
    """X [n, D] and one C [k, D] per run, uniform integers in [-4, 4] as fp32.  Uniform data alone
    ties on 1-7 % of the rows, so ties are planted: every odd centroid j is centroid j - 1 moved by
    2 (towards 0) in ONE random dim, and a quarter of the rows (at random positions) are a row
    near some even centroid of the run with the most centroids (``tie_run``) sitting midway
    between that pair in that dim: exactly equidistant from both, whatever its other coordinates
    (measured: ~30 % of the rows tie at every shape).  ``dup``: the last centroid of every run with
    k >= 2 repeats its first one."""
    g = torch.Generator().manual_seed(seed)
    X = torch.randint(-4, 5, (n, D), generator=g)
    Cs, dims = [], []
    for k in ks:
        C = torch.randint(-4, 5, (k, D), generator=g)
        dstar = torch.randint(0, D, (k // 2,), generator=g)
        for m in range(k // 2):
            C[2 * m + 1] = C[2 * m]
            C[2 * m + 1, dstar[m]] += 2 if int(C[2 * m, dstar[m]]) <= 0 else -2
        if dup and k >= 2:
            C[k - 1] = C[0]
        Cs.append(C.float())
        dims.append(dstar)
    r = tie_run(ks)
    C, dstar = Cs[r].long(), dims[r]
    if C.shape[0] >= 2:
        rows = torch.nonzero(torch.rand(n, generator=g) < 0.25).view(-1)
        m = torch.randint(0, C.shape[0] // 2, (rows.numel(),), generator=g)
        t, ar = rows.numel(), torch.arange(rows.numel())
        near = C[2 * m] + torch.randint(-1, 2, (t, D), generator=g) * (torch.rand((t, D), generator=g) < 0.2)
        near[ar, dstar[m]] = (C[2 * m] + C[2 * m + 1])[ar, dstar[m]] // 2
        X[rows] = near.clamp(-4, 4)
    return X.float(), Cs


def int_reference(X: torch.Tensor, C: torch.Tensor, chunk: int = 32768):
    """int64 reference of one Lloyd pass: (assign [n] lowest index on ties, counts [k], sums [k, D],
    sse, number of rows whose minimum is attained more than once).  The squared distances are
    ||x||^2 - 2 x.c + ||c||^2 in fp64, exact for these integers."""
    n, k = X.shape[0], C.shape[0]
    Xd, Cd = X.double(), C.double()
    cn = (Cd * Cd).sum(1)
    ar = torch.arange(k)
    assign = torch.empty(n, dtype=torch.long)
    sse, ties = 0, 0
    for s in range(0, n, chunk):
        xc = Xd[s:s + chunk]
        d2 = ((xc * xc).sum(1, keepdim=True) - 2.0 * (xc @ Cd.T) + cn).round().long()
        dmin = d2.min(1, keepdim=True).values
        hit = d2 == dmin
        assign[s:s + chunk] = torch.where(hit, ar, k).min(1).values
        sse += int(dmin.sum())
        ties += int((hit.sum(1) > 1).sum())
    counts = torch.bincount(assign, minlength=k)
    sums = torch.zeros((k, X.shape[1]), dtype=torch.long).index_add_(0, assign, X.long())
    return assign, counts, sums, sse, ties


def run_step(X: torch.Tensor, Cs: list[torch.Tensor]):
    """One fused Lloyd pass through the native entry points (as ``kmeans_step``), keeping the
    launched grid: ([(sums f64 [k, D], counts f64 [k], sse f64, assign int32 [n])], grid)."""
    from avenir_amd import _native
    from avenir_amd.models.cluster import _PairLayout
    D = X.shape[1]
    lay = _PairLayout(Cs, D)
    C = _native.C()
    partial, ssep, assign = C.kmeans_assign(X.float().contiguous(), lay.C2, lay.Cn, lay.roff, lay.h_roff, True)
    flat = C.kmeans_reduce(partial, ssep)
    out = []
    for r in range(len(Cs)):
        sums, counts, sse = lay.stats(flat, r, D)
        out.append((sums.cpu(), counts.cpu(), float(sse), assign[r].cpu()))
    return out, int(partial.shape[0])


def check_exact(X: torch.Tensor, Cs: list[torch.Tensor], dev, tag: str, lds: bool = False,
                min_tiles: int = 0) -> list[str]:
    """Battery A on one launch: bit-exact assign / counts / sums / sse per run against the int64
    reference, and (from the reference alone) exact ties on >= 5 % of the rows of the run the ties
    were planted for when it has k >= 2 and n >= 257 rows.  ``min_tiles``: additionally require
    that every wave (LDS kernel: thread) of the LAUNCHED grid walks at least that many tiles (rows)
    plus a ragged tail."""
    fails = []
    n = X.shape[0]
    got, grid = run_step(X.to(dev), [C.to(dev) for C in Cs])
    if min_tiles:
        have, need = (n, min_tiles * 256 * grid + 1) if lds else (-(-n // 64), min_tiles * 4 * grid + 1)
        if have < need:
            fails.append(f"{tag}: grid {grid} is too large for n {n}: {have} tiles (rows) < {need}; no wave runs "
                         f"{min_tiles} tiles, pick a larger n for this machine")
    for r, (C, (sums, counts, sse, assign)) in enumerate(zip(Cs, got)):
        k = C.shape[0]
        ra, rc, rs, rsse, ties = int_reference(X, C)
        t = f"{tag} run {r} (k {k})"
        planted = r == tie_run([c.shape[0] for c in Cs]) and k >= 2 and n >= TIE_N
        if planted and ties < MIN_TIE_SHARE * n:
            fails.append(f"{t}: only {ties} of {n} rows tie exactly; the data does not exercise the tie rule")
        a = assign.long()
        if not torch.equal(a, ra):
            bad = torch.nonzero(a != ra).view(-1)
            i = int(bad[0])
            fails.append(f"{t}: {bad.numel()} of {n} assignments differ, first row {i}: got {int(a[i])} "
                         f"want {int(ra[i])}")
        if not torch.equal(counts.long(), rc) or not torch.equal(counts, rc.double()):
            fails.append(f"{t}: counts differ: got {counts.tolist()[:8]} want {rc.tolist()[:8]}")
        if not torch.equal(sums, rs.double()):
            fails.append(f"{t}: sums differ, max abs {float((sums - rs.double()).abs().max())}")
        if sse != float(rsse):
            fails.append(f"{t}: sse {sse!r} != {rsse}")
    return fails


def battery(shape, dev, ns=SMALL_N, lds: bool = False, dup: bool = False) -> list[str]:
    """Battery A of one (D, k) or (D, [k...]) shape at the small row counts."""
    D, ks = shape
    ks = [ks] if isinstance(ks, int) else list(ks)
    fails = []
    for n in ns:
        X, Cs = int_data(n, D, ks, seed=1000 * D + 7 * sum(ks) + n, dup=dup)
        fails += check_exact(X, Cs, dev, f"D {D} k {ks} n {n}" + (" dup" if dup else ""), lds=lds)
    return fails


def battery_big(shape, dev, lds: bool = False) -> list[str]:
    """Battery A at BIG_N: every wave rotates through >= 3 tiles and the tail tile is ragged."""
    D, ks = shape
    ks = [ks] if isinstance(ks, int) else list(ks)
    X, Cs = int_data(BIG_N, D, ks, seed=31 * D + sum(ks))
    return check_exact(X, Cs, dev, f"D {D} k {ks} n {BIG_N}", lds=lds, min_tiles=3)


# ----------------------------------------------------------------------------------------------
# C: partial sums are fp32-exact
SUMS_N, SUMS_K = 4096, 16
Q = 2.0 ** -19


def sums_data(D: int, scale: float, seed: int = 0):
    """X [4096, D], C [16, D] (fp32, exact), labels: row r is cluster r mod 16; every coordinate a
    multiple of 2^-19 in [1, 2): a random 20-bit centre per (cluster, dim) plus a per-row jitter of
    at most 2^-5, clamped to the interval; all times ``scale`` (a power of two)."""
    g = torch.Generator().manual_seed(seed + D)
    C = 1.0 + torch.randint(0, 1 << 19, (SUMS_K, D), generator=g).double() * Q
    lab = torch.arange(SUMS_N) % SUMS_K
    jit = torch.randint(-(1 << 14), (1 << 14) + 1, (SUMS_N, D), generator=g).double() * Q
    X = (C[lab] + jit).clamp(1.0, 2.0 - Q)
    Xf, Cf = (X * scale).float(), (C * scale).float()
    assert torch.equal(Xf.double(), X * scale) and torch.equal(Cf.double(), C * scale)
    return Xf, Cf, lab


def sums_margin_ok(X: torch.Tensor, C: torch.Tensor, lab: torch.Tensor, scale: float) -> list[str]:
    """Reference-only precondition: the fp64 nearest centre is the row's own and the second
    nearest is further by more than any mode's scoring error.  The coarsest mode (split-bf16 x3)
    drops the x2 / c2 terms and the x1.c1 product: <= 2^-15 relative per product, products <=
    (2 scale)^2, D of them, twice in ||c||^2 - 2 x.c, for two centroids: D 2^-11 scale^2.  Four
    times that is required."""
    d2 = torch.cdist(X.double(), C.double()) ** 2
    two = d2.topk(2, dim=1, largest=False)
    fails = []
    if not torch.equal(two.indices[:, 0], lab):
        fails.append("sums data: a row's fp64 nearest centre is not its own")
    need = 4 * X.shape[1] * 2.0 ** -11 * scale * scale
    margin = float((two.values[:, 1] - two.values[:, 0]).min())
    if margin < need:
        fails.append(f"sums data: fp64 margin {margin} < {need}")
    return fails


def check_sums(D: int, scale: float, dev, kind: str = "score") -> list[str]:
    """C on one shape.  kind: 'score' (one run), 'mfma' (the same centres as two runs), 'lds'
    (k = 300: the 16 centres plus 284 far-away ones)."""
    X, C, lab = sums_data(D, scale)
    fails = sums_margin_ok(X, C, lab, scale)
    if kind == "lds":
        g = torch.Generator().manual_seed(5)
        far = (8.0 + torch.randint(0, 1 << 10, (284, D), generator=g).double() / 128.0) * scale
        Cs = [torch.cat([C, far.float()])]
    else:
        Cs = [C, C] if kind == "mfma" else [C]
    got, _ = run_step(X.to(dev), [c.to(dev) for c in Cs])
    ref = torch.zeros((SUMS_K, D), dtype=torch.float64).index_add_(0, lab, X.double())
    for r, (sums, counts, _, assign) in enumerate(got):
        t = f"sums {kind} D {D} scale {scale:g} run {r}"
        if not torch.equal(assign.long(), lab):
            fails.append(f"{t}: {int((assign.long() != lab).sum())} rows not assigned to their own centre")
            continue
        if not torch.equal(counts[:SUMS_K], torch.full((SUMS_K,), SUMS_N / SUMS_K, dtype=torch.float64)):
            fails.append(f"{t}: counts {counts[:SUMS_K].tolist()}")
        err = (sums[:SUMS_K] - ref).abs()
        if not torch.equal(sums[:SUMS_K], ref):
            fails.append(f"{t}: {int((err > 0).sum())} of {err.numel()} sums are not the exact fp64 sum, max abs "
                         f"error {float(err.max()):.6g} = {float(err.max()) / (Q * scale):.1f} quanta of 2^-19 scale")
        if bool((sums[SUMS_K:] != 0).any()) or bool((counts[SUMS_K:] != 0).any()):
            fails.append(f"{t}: a far-away centre received rows")
    return fails


SUMS_SCALES = (1.0, 2.0 ** 13)
SUMS_SCORE_D = (8, 16, 32)


def child_main() -> int:
    """Battery A on the score-kernel shapes (small n and BIG_N) and C on the score kernel, in THIS
    process's AVMI_KMEANS_* mode; one JSON line; exit status 1 on any failure."""
    t0 = time.monotonic()
    dev = torch.device("cuda")
    fails = []
    for shape in SCORE_SHAPES:
        fails += battery(shape, dev)
        fails += battery_big(shape, dev)
    fails += battery((16, 16), dev, dup=True)
    for D in SUMS_SCORE_D:
        for scale in SUMS_SCALES:
            fails += check_sums(D, scale, dev, "score")
    torch.cuda.synchronize()
    mode = {k: v for k, v in os.environ.items() if k.startswith("AVMI_KMEANS_")}
    print(json.dumps({"ok": not fails, "mode": mode, "failures": fails[:20], "n_failures": len(fails),
                      "seconds": round(time.monotonic() - t0, 2)}))
    return 1 if fails else 0


if __name__ == "__main__":
    sys.exit(child_main())
