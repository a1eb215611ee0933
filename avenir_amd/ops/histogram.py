"""Counting ops (K2/K3/K4/moments).  GPU tensors -> hand-written HIP kernels (``_C``);
CPU tensors -> the PyTorch reference implementation of the same op (golden oracle)."""
from __future__ import annotations

import os

from dataclasses import dataclass
from typing import Sequence

import torch

from .. import _native


_CONST_CACHE: dict = {}


def _dev_i32(vals: Sequence[int], device) -> torch.Tensor:
    """Small int32 metadata tensors, cached per (values, device) so repeated launches do not pay a
    host->device copy (and its implicit synchronisation) every call."""
    key = (tuple(int(v) for v in vals), str(device))
    t = _CONST_CACHE.get(key)
    if t is None:
        if len(_CONST_CACHE) > 4096:
            _CONST_CACHE.clear()
        t = torch.tensor(list(key[0]), dtype=torch.int32, device=device)
        _CONST_CACHE[key] = t
    return t


def class_histogram(codes: torch.Tensor, n: int, bins: Sequence[int], labels: torch.Tensor | None,
                    n_classes: int, out: torch.Tensor | None = None, mode: int = 0,
                    count_labels: bool = False) -> torch.Tensor:
    """Class-conditional histogram ``out[c, off_f + b]`` (int64 ``[C, sum(bins)]``; with
    ``count_labels`` an extra last column holds the per-class record counts, fused in the same
    pass so no host synchronisation is needed).

    ``codes`` uint8 ``[F, ld]`` (feature-major), codes >= bins[f] (e.g. 255) are skipped;
    ``labels`` uint8 ``[>= n]`` or None (then C = 1).  ``mode``: 0 auto (packed byte-counter fast
    path when C*bins <= 16), 1 LDS path, 2 global-atomic path (for tests).
    """
    F = codes.shape[0]
    bins = [int(b) for b in bins]
    assert len(bins) == F, "bins length must equal number of feature rows"
    tb = sum(bins) + (1 if count_labels else 0)
    C = int(n_classes) if labels is not None else 1
    if out is None:
        out = torch.zeros((C, tb), dtype=torch.int64, device=codes.device)
    if (F == 0 and not count_labels) or n == 0:
        return out
    if codes.is_cuda:
        offs = [0] * F
        for f in range(1, F):
            offs[f] = offs[f - 1] + bins[f - 1]
        _native.C().class_histogram(codes.contiguous(), int(n),
                                    None if labels is None else labels.contiguous(),
                                    _dev_i32(bins, codes.device), _dev_i32(offs, codes.device),
                                    bins, tb, C, out, int(mode), bool(count_labels))
        return out
    # --- CPU reference ---
    lab = labels[:n].long() if labels is not None else torch.zeros(n, dtype=torch.long)
    if count_labels:
        ok = lab < C
        out[:, tb - 1] += torch.bincount(lab[ok], minlength=C)[:C]
    o = 0
    for f, b in enumerate(bins):
        v = codes[f, :n].long()
        ok = (v < b) & (lab < C)
        idx = lab[ok] * b + v[ok]
        out[:, o:o + b] += torch.bincount(idx, minlength=C * b).view(C, b)
        o += b
    return out


# ------------------------------------------------------------------------------------------------
# row-packed records: every categorical code of a record and its class in ONE 16-bit word
# ------------------------------------------------------------------------------------------------
@dataclass
class RowPacked:
    """Records packed one 16-bit word each (``pack_rows``): feature k's code in bits
    [shifts[k], shifts[k] + widths[k]) (its all-ones value = missing code); for C = 2 the class
    as two one-hot bits at label_shift (bit c set = class c, none set = unknown class)."""
    words: torch.Tensor      # int16 [>= n], numel a multiple of 8 (16-byte vector loads)
    n: int
    bins: list[int]
    shifts: list[int]
    widths: list[int]
    label_shift: int
    label_width: int         # 0: no class field (C = 1)
    n_classes: int
    dense: torch.Tensor | None = None   # GPU: the same records as a dense B-bit stream (see ensure_dense)
    bits: int = 16                      # B: bits per record of ``dense`` (of the word's fields without one)
    radices: list[int] | None = None    # mixed-radix digits of the features (``radix_layout``)
    class_radix: int = 1                # 1: no class digit (C = 1); 2; 3: digit 2 = unknown class
    dense_is_radix: bool = False        # ``dense`` holds mixed-radix codes, not the bit-field records
    field_bits: int | None = None       # bits of the bit-field record when ``bits`` counts the radix code
    bitfield: torch.Tensor | None = None  # the bit-field stream next to a radix ``dense`` (built on first use)
    # the patched stream next to a radix ``dense`` (``attach_patched``; GPU only, None where it does not pay)
    patched: torch.Tensor | None = None   # the records' cells, ``patched_bits`` each, in the container of ``dense``
    patched_bits: int | None = None       # b < bits; ESC = 2^b - 1 marks a record listed in the exceptions
    exc_index: torch.Tensor | None = None  # int64 [E], ascending: the records that store ESC
    exc_cell: torch.Tensor | None = None   # int16 [E]: their cells (> ESC)
    cell_state: torch.Tensor | None = None  # int16 [J + 1]: state of a cell, -1 for cell ESC
    state_cell: torch.Tensor | None = None  # int16 [J]: cell of a state

    def ensure_dense(self) -> "RowPacked":
        """Attach the dense B-bit stream (32 records per B dwords) the joint-table kernels stream
        instead of the 16-bit words; GPU only, B in 4..15.  With ``radices`` set and
        ceil(log2 J) in 4..15 the records are mixed-radix codes (churn: 11 bits, 1.375 B/record),
        else the word's bit fields back to back (churn: 13 bits)."""
        if self.dense is not None or not self.words.is_cuda or self.n <= 0:
            return self
        if self.radices is not None:
            tb = sum(self.bins) + 1
            _, B, _ = _native.C().radix_shape(list(self.radices), int(self.class_radix), int(self.n_classes), tb)
            if 4 <= B <= 15:
                self.dense = _native.C().pack_radix(self.words, int(self.n), int(B), list(self.shifts),
                                                    list(self.widths), list(self.radices), list(self.bins),
                                                    int(self.label_shift), int(self.class_radix),
                                                    int(self.n_classes))
                self.field_bits, self.bits, self.dense_is_radix = self.bits, int(B), True
                attach_patched(self)
                return self
        if 4 <= self.bits <= 15:
            self.dense = _native.C().pack_dense(self.words, int(self.n), int(self.bits))
        return self

    def ensure_bitfield(self) -> torch.Tensor | None:
        """The bit-field stream of the records (AVMI_ROWPACK_KERNEL=bitfield): ``dense`` itself
        unless that holds mixed-radix codes; then packed from the words on first use."""
        if not self.dense_is_radix:
            return self.dense
        if self.bitfield is None and 4 <= self.field_bits <= 15:
            self.bitfield = _native.C().pack_dense(self.words, int(self.n), int(self.field_bits))
        return self.bitfield


def radix_layout(bins: Sequence[int], n_classes: int, missing: Sequence[bool] | None = None,
                 unknown: bool = True, count_labels: bool = True):
    """Mixed-radix code of a record, class digit least significant, then feature 0, 1, ...:
    feature k's digit is its code, of radix bins[k], or bins[k] + 1 with the missing code as digit
    bins[k] when ``missing[k]``; the class digit (C = 2 only) is the class, of radix 2, or 3 with
    digit 2 for an unknown class when ``unknown``.  Returns (radices, class_radix, J, B, R): the
    joint states, B = ceil(log2 J) bits per record and the replicas of the J-cell table the kernel
    keeps in LDS next to the [C, sum(bins) (+1)] table; None when B is outside 4..15 (no stream)."""
    bins = [int(b) for b in bins]
    C = int(n_classes)
    if missing is None:
        missing = [True] * len(bins)
    if not bins or len(bins) > 8 or C < 1 or C > 2 or min(bins) < 1 or max(bins) > 8:
        return None
    radices = [b + 1 if m else b for b, m in zip(bins, missing)]
    class_radix = 1 if C == 1 else (3 if unknown else 2)
    tb = sum(bins) + (1 if count_labels else 0)
    J, B, R = _native.C().radix_shape(radices, class_radix, C, tb)
    if not 4 <= B <= 15:
        return None
    return radices, class_radix, int(J), int(B), int(R)


# ------------------------------------------------------------------------------------------------
# patched record stream: b < B = ceil(log2 J) bits per record beside the B-bit mixed-radix stream.
# A record whose state is among the 2^b - 1 most frequent stores that state's frequency rank; any
# other stores ESC = 2^b - 1 and is listed as (record index, cell) in the exception lists.  The cell
# of rank r is r below ESC and r + 1 from ESC on, so J + 1 cells (cell ESC a dummy) index one joint
# table.  ``ref_patch_encode`` / ``ref_patch_decode`` define the format; the HIP packer equals them
# bit for bit (tests/test_rowpack_patched.py).
# ------------------------------------------------------------------------------------------------
PATCH_SAMPLE = 1 << 20     # records of the strided sample the states are ranked from
# A patched stream is kept while its kernel bytes (stream + 2 per exception) stay below PATCH_MARGIN
# times the plain stream's.  profiles/patched_cap_sweep.jsonl (benchmarks/bench_patched_sweep.py, 2^28
# churn-shaped records, 10 against 11 bits): patched won every repetition up to 2 % escaped records,
# a byte ratio of 0.9372; at 4 % (0.9622) only the median won, at 8 % (1.0173) the plain stream did.
PATCH_MARGIN = 0.937


def patch_ranks(counts) -> torch.Tensor:
    """int64 [J]: frequency rank of every state, by descending count, ties by ascending code."""
    c = torch.as_tensor(counts, dtype=torch.int64).cpu()
    order = torch.sort(-c, stable=True).indices
    rank = torch.empty_like(order)
    rank[order] = torch.arange(c.numel())
    return rank


def patch_tables(counts, b: int) -> tuple[torch.Tensor, torch.Tensor]:
    """(state_cell int16 [J], cell_state int16 [J + 1]) at width b; cell ESC maps to no state (-1)."""
    rank = patch_ranks(counts)
    J, esc = rank.numel(), (1 << int(b)) - 1
    if not 4 <= int(b) <= 14 or esc + 1 >= J or J + 1 > 1 << 15:
        raise ValueError("patched stream: 4 <= b < ceil(log2 J), b <= 14, J + 1 <= 2^15")
    state_cell = torch.where(rank < esc, rank, rank + 1)
    cell_state = torch.full((J + 1,), -1, dtype=torch.int64)
    cell_state[state_cell] = torch.arange(J)
    return state_cell.to(torch.int16), cell_state.to(torch.int16)


def patch_cost(counts, b: int) -> float:
    """Estimated kernel bytes per record at width b: b / 8 + 2 p_exc(b)."""
    c = torch.as_tensor(counts, dtype=torch.int64).cpu()
    top = torch.sort(c, descending=True).values
    return b / 8.0 + 2.0 * float(top[(1 << b) - 1:].sum()) / max(1, int(c.sum()))


def choose_patch_bits(counts, margin: float = PATCH_MARGIN) -> int | None:
    """The width b in [4, B - 1] of the least estimated bytes per record (the smaller b on a tie),
    or None when no width stays below ``margin`` * B / 8 or the layout has no patched stream."""
    J = int(torch.as_tensor(counts).numel())
    B = max(0, J - 1).bit_length()
    if J + 1 > 1 << 15 or int(torch.as_tensor(counts).sum()) <= 0:
        return None
    best = None
    for b in range(4, min(B, 15)):
        cost = patch_cost(counts, b)
        if best is None or cost < best[0]:
            best = (cost, b)
    if best is None or not best[0] < margin * B / 8.0:
        return None
    return best[1]


def patch_keep(b: int, B: int, n: int, n_exc: int, margin: float = PATCH_MARGIN) -> bool:
    """The decision after packing, with the exact exception count: the kernel reads the stream and
    two bytes per exception."""
    groups = (int(n) + 31) // 32
    return b * groups * 4 + 2 * int(n_exc) < margin * (B * groups * 4)


def _pack_bits(v: torch.Tensor, B: int) -> torch.Tensor:
    """int32 [ceil(n / 32) * B]: value k of group g at bits [k B, k B + B) of the group's B dwords."""
    v = v.long().cpu()
    n = v.numel()
    r = torch.arange(n)
    pos = (r // 32) * (32 * B) + (r % 32) * B
    acc = torch.zeros((n + 31) // 32 * B, dtype=torch.int64)
    for i in range(B):
        acc.index_add_(0, (pos + i) // 32, ((v >> i) & 1) << ((pos + i) % 32))
    return torch.where(acc >= 1 << 31, acc - (1 << 32), acc).to(torch.int32)


def _unpack_bits(dense: torch.Tensor, n: int, B: int) -> torch.Tensor:
    d = dense.long().cpu() & 0xFFFFFFFF
    r = torch.arange(n)
    pos = (r // 32) * (32 * B) + (r % 32) * B
    v = torch.zeros(n, dtype=torch.int64)
    for i in range(B):
        v |= ((d[(pos + i) // 32] >> ((pos + i) % 32)) & 1) << i
    return v


def ref_patch_encode(code: torch.Tensor, state_cell: torch.Tensor, b: int):
    """CPU twin of the packer: (stream int32, exc_index int64 ascending, exc_cell int16) of the
    mixed-radix codes ``code`` int64 [n]."""
    cell = state_cell.long().cpu()[code.long().cpu()]
    esc = (1 << int(b)) - 1
    out = cell > esc
    stream = _pack_bits(torch.where(out, torch.full_like(cell, esc), cell), int(b))
    return stream, out.nonzero().flatten(), cell[out].to(torch.int16)


def ref_patch_decode(stream: torch.Tensor, n: int, b: int, exc_index: torch.Tensor, exc_cell: torch.Tensor,
                     cell_state: torch.Tensor) -> torch.Tensor:
    """Inverse of ``ref_patch_encode``: the int64 [n] mixed-radix codes."""
    cell = _unpack_bits(stream, int(n), int(b))
    esc = (1 << int(b)) - 1
    idx = exc_index.long().cpu()
    assert torch.equal((cell == esc).nonzero().flatten(), idx), "the exceptions are the records that store ESC"
    cell[idx] = exc_cell.long().cpu() & 0xFFFF
    return cell_state.long().cpu()[cell]


def _radix_codes(rp: "RowPacked", words: torch.Tensor) -> torch.Tensor:
    """int64 mixed-radix codes of 16-bit ``words`` in the layout of ``rp`` (as the packer kernels:
    every digit clamped to its radix)."""
    w = words.to(torch.int64) & 0xFFFF
    code = torch.zeros_like(w)
    mult = 1
    if rp.class_radix > 1:
        lb = (w >> rp.label_shift) & 3
        cd = torch.where(lb == 1, torch.zeros_like(lb), torch.where(lb == 2, torch.ones_like(lb), torch.full_like(lb, 2)))
        code = cd.clamp_max(rp.class_radix - 1)
        mult = rp.class_radix
    for s, wd, r in zip(rp.shifts, rp.widths, rp.radices):
        code = code + ((w >> s) & ((1 << wd) - 1)).clamp_max(r - 1) * mult
        mult *= r
    return code


def attach_patched(rp: "RowPacked", bits: int | None = None, sample: torch.Tensor | None = None,
                   margin: float | None = None) -> "RowPacked":
    """Build the patched stream of ``rp`` next to its mixed-radix stream (GPU only), or leave none
    where it does not pay.  The states are ranked from a strided sample of at most PATCH_SAMPLE
    records (``sample``: record indices to rank from instead); the width is ``choose_patch_bits``
    of the sample and the stream is kept when ``patch_keep`` holds for the exact exception count.
    ``bits`` forces a width and keeps the stream whatever it costs (tests, the margin sweep)."""
    rp.patched = rp.patched_bits = rp.exc_index = rp.exc_cell = rp.cell_state = rp.state_cell = None
    if not rp.dense_is_radix or not rp.words.is_cuda or rp.n <= 0:
        return rp
    margin = PATCH_MARGIN if margin is None else float(margin)
    J = int(rp.class_radix)
    for r in rp.radices:
        J *= int(r)
    B = int(rp.bits)
    if B < 5 or J + 1 > 1 << 15:
        return rp
    picked = rp.words[:rp.n:-(-rp.n // PATCH_SAMPLE)] if sample is None else rp.words[sample]
    counts = torch.bincount(_radix_codes(rp, picked), minlength=J).cpu()
    if bits is None:
        b = choose_patch_bits(counts, margin)
        if b is None:
            return rp
    else:
        b = int(bits)
        if not 4 <= b < B:
            raise ValueError("patched stream: 4 <= bits < ceil(log2 J)")
    state_cell, cell_state = patch_tables(counts, b)
    dev = rp.words.device
    state_cell, cell_state = state_cell.to(dev), cell_state.to(dev)
    lay = (int(rp.n), b, list(rp.shifts), list(rp.widths), list(rp.radices), list(rp.bins), int(rp.label_shift),
           int(rp.class_radix), int(rp.n_classes), state_cell)
    stream, n_exc = _native.C().pack_patched(rp.words, *lay)
    E = int(n_exc.item())
    if bits is None and not patch_keep(b, B, rp.n, E, margin):
        return rp                        # the sample misled: the plain stream is the shorter read
    idx, cell = _native.C().patch_exceptions(rp.words, *lay, E)
    if E:                                # the kernel appends in any order: the same bits on every run
        idx, order = torch.sort(idx)
        cell = cell[order]
    rp.patched, rp.patched_bits, rp.exc_index, rp.exc_cell = stream, b, idx, cell
    rp.cell_state, rp.state_cell = cell_state, state_cell
    return rp


def rowpack_layout(bins: Sequence[int], n_classes: int, missing: Sequence[bool] | None = None):
    """(shifts, widths, label_shift, label_width) of the 16-bit record, or None when the schema
    does not fit: at most 8 features of at most 3 bits and 1 or 2 classes (C = 2: two one-hot
    class bits).  A feature with missing values takes bit_length(b) bits so its all-ones value
    (>= b) is free for 'missing'; one without (``missing[k]`` False) only bit_length(b - 1)."""
    bins = [int(b) for b in bins]
    C = int(n_classes)
    if missing is None:
        missing = [True] * len(bins)
    if not bins or len(bins) > 8 or C < 1 or C > 2 or min(bins) < 1:
        return None
    widths = [max(1, (b if m else b - 1).bit_length()) for b, m in zip(bins, missing)]
    if max(widths) > 3:
        return None
    lw = 2 if C == 2 else 0            # C = 2: class bits 0-1, the fields from bit 2
    shifts, s = [], lw
    for w in widths:
        shifts.append(s)
        s += w
    if s > 16:
        return None
    return shifts, widths, 0 if lw else s, lw


def pack_rows(codes: torch.Tensor, n: int, bins: Sequence[int], labels: torch.Tensor | None,
              n_classes: int) -> RowPacked | None:
    """Pack ``codes`` uint8 [F, >= n] (+ ``labels``) into one 16-bit word per record, on the
    tensors' device; None when ``rowpack_layout`` refuses the schema.  Codes >= bins[k] and
    labels >= C become the field's all-ones value, which every consumer skips — exactly the
    records the column histogram skips, so the counts are identical."""
    bins = [int(b) for b in bins]
    C = int(n_classes) if labels is not None else 1
    if labels is not None and C == 1:
        return None                      # a 1-class label column still filters rows: keep columns
    if codes.shape[0] != len(bins):
        return None
    # data-adaptive widths: a feature without missing codes needs no all-ones 'missing' value
    missing = [bool((codes[k, :n] >= b).any()) for k, b in enumerate(bins)] if n else [False] * len(bins)
    lay = rowpack_layout(bins, C, missing)
    if lay is None:
        return None
    shifts, widths, lsh, lw = lay
    w = torch.zeros(max(8, (n + 7) // 8 * 8), dtype=torch.int32, device=codes.device)
    body = w[:n]
    for k, (b, s, wd) in enumerate(zip(bins, shifts, widths)):
        v = codes[k, :n].to(torch.int32)
        body |= torch.where(v < b, v, torch.full_like(v, (1 << wd) - 1)) << s
    if lw:
        v = labels[:n].to(torch.int32)
        body |= torch.where(v < C, 1 << v.clamp_max(C - 1), torch.zeros_like(v)) << lsh
    words = torch.where(w >= 32768, w - 65536, w).to(torch.int16)
    bits = max([s + wd for s, wd in zip(shifts, widths)] + [lsh + lw])
    # mixed-radix digits (radix_layout): a missing / unknown digit only where the data holds one
    unknown = bool((labels[:n] >= C).any()) if lw and n else False
    radices = [b + 1 if m else b for b, m in zip(bins, missing)]
    return RowPacked(words, int(n), bins, shifts, widths, lsh, lw, C, bits=bits, radices=radices,
                     class_radix=1 if C == 1 else (3 if unknown else 2)).ensure_dense()


def unpack_rows(rp: RowPacked) -> tuple[torch.Tensor, torch.Tensor | None]:
    """Inverse of ``pack_rows``: (codes uint8 [F, pad16(n)], labels uint8 [pad16(n)] or None),
    missing / unknown values as 255."""
    n = rp.n
    ld = max(16, (n + 15) // 16 * 16)
    w = rp.words[:n].to(torch.int32) & 0xFFFF
    codes = torch.full((len(rp.bins), ld), 255, dtype=torch.uint8, device=w.device)
    for k, (b, s, wd) in enumerate(zip(rp.bins, rp.shifts, rp.widths)):
        v = (w >> s) & ((1 << wd) - 1)
        codes[k, :n] = torch.where(v < b, v, torch.full_like(v, 255)).to(torch.uint8)
    labels = None
    if rp.label_width:
        labels = torch.full((ld,), 255, dtype=torch.uint8, device=w.device)
        v = (w >> rp.label_shift) & ((1 << rp.label_width) - 1)
        cls = torch.full_like(v, 255)                                     # one-hot class bits
        for c in range(rp.n_classes):
            cls = torch.where(v == (1 << c), torch.full_like(v, c), cls)
        labels[:n] = cls.to(torch.uint8)
    return codes, labels


def class_histogram_packed(rp: RowPacked, out: torch.Tensor | None = None,
                           count_labels: bool = False) -> torch.Tensor:
    """``class_histogram`` over row-packed records (same ``[C, sum(bins) (+1)]`` int64 result).
    GPU: the K2 joint-table kernel streams the records' dense stream (``ensure_dense``: mixed-radix
    codes, else bit fields; the patched stream where ``attach_patched`` kept one), or the 16-bit
    words, instead of F + 1 bytes of code columns; AVMI_ROWPACK_KERNEL=radix / bitfield / joint /
    nibble select the plain mixed-radix stream, the bit-field stream and the two word kernels.
    CPU: unpack + the column reference."""
    C = rp.n_classes
    tb = sum(rp.bins) + (1 if count_labels else 0)
    if out is None:
        out = torch.zeros((C, tb), dtype=torch.int64, device=rp.words.device)
    if rp.n == 0:
        return out
    if rp.words.is_cuda:
        offs = [0] * len(rp.bins)
        for f in range(1, len(rp.bins)):
            offs[f] = offs[f - 1] + rp.bins[f - 1]
        # kernel order: features of <= 2 bits first (for C = 2 they share one counter per record
        # across both classes); output columns stay in schema order through offs
        order = sorted(range(len(rp.bins)), key=lambda k: (C == 2 and rp.widths[k] > 2, k))
        dev = rp.words.device
        kind = os.environ.get("AVMI_ROWPACK_KERNEL", "dense")
        if kind == "dense" and rp.patched is not None:
            # patched records: the same hot loop over fewer bits, the exception list added after it
            _native.C().class_histogram_patched(rp.patched, int(rp.n), int(rp.patched_bits), list(rp.radices),
                                                list(rp.bins), offs, int(rp.class_radix), tb, C, out,
                                                bool(count_labels), rp.exc_cell, rp.cell_state)
            return out
        if kind in ("dense", "radix") and rp.dense_is_radix:
            # mixed-radix records: the code is the cell of the J-cell joint table, one LDS atomic per record
            _native.C().class_histogram_radix(rp.dense, int(rp.n), int(rp.bits), list(rp.radices), list(rp.bins),
                                              offs, int(rp.class_radix), tb, C, out, bool(count_labels))
            return out
        stream = rp.ensure_bitfield() if kind in ("dense", "radix", "bitfield") else None
        if stream is not None:
            # bit-field records back to back, one LDS atomic per record into the 2^bits joint table
            fb = rp.field_bits if rp.dense_is_radix else rp.bits
            _native.C().class_histogram_dense(stream, int(rp.n), int(fb), list(rp.shifts), list(rp.widths),
                                              rp.label_shift, rp.label_width, _dev_i32(rp.bins, dev),
                                              _dev_i32(offs, dev), tb, C, out, bool(count_labels),
                                              list(rp.bins), offs)
            return out
        _native.C().class_histogram_rowpacked(rp.words, int(rp.n), [rp.shifts[k] for k in order],
                                              [rp.widths[k] for k in order], rp.label_shift, rp.label_width,
                                              _dev_i32([rp.bins[k] for k in order], dev),
                                              _dev_i32([offs[k] for k in order], dev), tb, C, out,
                                              bool(count_labels))
        return out
    codes, labels = unpack_rows(rp)
    return class_histogram(codes, rp.n, rp.bins, labels, C, out=out, count_labels=count_labels)


def pair_histogram(codes: torch.Tensor, n: int, bins: Sequence[int],
                   pairs: Sequence[tuple[int, int]], labels: torch.Tensor | None,
                   n_classes: int) -> list[torch.Tensor]:
    """Joint histograms for feature pairs: list of int64 ``[C, B_a, B_b]`` tensors."""
    bins = [int(b) for b in bins]
    C = int(n_classes) if labels is not None else 1
    sizes = [C * bins[a] * bins[b] for a, b in pairs]
    if not pairs:
        return []
    if codes.is_cuda:
        offs = [0] * len(pairs)
        for i in range(1, len(pairs)):
            offs[i] = offs[i - 1] + sizes[i - 1]
        flat = torch.zeros(sum(sizes), dtype=torch.int64, device=codes.device)
        pt = torch.tensor([list(p) for p in pairs], dtype=torch.int32, device=codes.device)
        po = torch.tensor(offs, dtype=torch.int64, device=codes.device)
        _native.C().pair_histogram(codes.contiguous(), int(n),
                                   None if labels is None else labels.contiguous(),
                                   _dev_i32(bins, codes.device), pt, po, max(sizes), C, flat)
        return [flat[o:o + s].view(C, bins[a], bins[b]) for o, s, (a, b) in zip(offs, sizes, pairs)]
    lab = labels[:n].long() if labels is not None else torch.zeros(n, dtype=torch.long)
    res = []
    for a, b in pairs:
        va, vb = codes[a, :n].long(), codes[b, :n].long()
        ok = (va < bins[a]) & (vb < bins[b]) & (lab < C)
        idx = (lab[ok] * bins[a] + va[ok]) * bins[b] + vb[ok]
        res.append(torch.bincount(idx, minlength=C * bins[a] * bins[b]).view(C, bins[a], bins[b]))
    return res


def bigram_histogram(states: torch.Tensor, n_states: int, labels: torch.Tensor | None = None,
                     n_classes: int = 1) -> torch.Tensor:
    """Markov transition counts ``[C, S, S]`` from int16 state sequences ``[N, L]`` (negative =
    padding)."""
    C = int(n_classes) if labels is not None else 1
    S = int(n_states)
    out = torch.zeros((C, S, S), dtype=torch.int64, device=states.device)
    if states.numel() == 0 or states.shape[1] < 2:
        return out
    if states.is_cuda:
        _native.C().bigram_histogram(states.to(torch.int16).contiguous(),
                                     None if labels is None else labels.contiguous(), C, S, out)
        return out
    a = states[:, :-1].long()
    b = states[:, 1:].long()
    lab = (labels[: states.shape[0]].long() if labels is not None
           else torch.zeros(states.shape[0], dtype=torch.long)).unsqueeze(1).expand_as(a)
    ok = (a >= 0) & (b >= 0) & (a < S) & (b < S) & (lab < C)
    idx = (lab[ok] * S + a[ok]) * S + b[ok]
    out += torch.bincount(idx, minlength=C * S * S).view(C, S, S)
    return out


def class_moments(x: torch.Tensor, n: int, labels: torch.Tensor | None, n_classes: int) -> torch.Tensor:
    """``[C, F, 3]`` float64 (count, sum, sum of squares) per class and continuous feature."""
    C = int(n_classes) if labels is not None else 1
    F = x.shape[0]
    if F == 0 or n == 0:
        return torch.zeros((C, F, 3), dtype=torch.float64, device=x.device)
    if x.is_cuda:
        return _native.C().class_moments(x.float().contiguous(), int(n),
                                         None if labels is None else labels.contiguous(), C)
    lab = labels[:n].long() if labels is not None else torch.zeros(n, dtype=torch.long)
    xv = x[:, :n].double()
    out = torch.zeros((C, F, 3), dtype=torch.float64)
    for c in range(C):
        m = lab == c
        xc = xv[:, m]
        out[c, :, 0] = float(m.sum())
        out[c, :, 1] = xc.sum(1)
        out[c, :, 2] = (xc * xc).sum(1)
    return out
