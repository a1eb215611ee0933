"""Patched record stream of the row-packed class histogram (``ops/histogram.py``): a record stores
the frequency rank of its joint state in b < B = ceil(log2 J) bits, or the escape code 2^b - 1 and an
entry in the exception lists.  CPU: the twin ``ref_patch_encode`` / ``ref_patch_decode`` is lossless,
the rank tables are what the format says, the width is chosen from a count vector as specified and a
misleading sample ends without a stream.  GPU: the HIP packer equals the twin bit for bit, and the
joint-table kernel's counts over the patched stream equal the column histogram
``H.class_histogram`` over sizes around the group / block boundaries, with and without exceptions,
for every replica count used, and a bad argument raises before any launch."""
import math

import pytest
import torch

from avenir_amd import _native
from avenir_amd.data.synth import _CHURN_W, CHURN_SCHEMA, churn_device
from avenir_amd.data.table import Table
from avenir_amd.models.bayes import NaiveBayes
from avenir_amd.ops import histogram as H
from avenir_amd.utils.schema import FeatureSchema

gpu = pytest.mark.gpu

CHURN = [4, 3, 3, 3, 5]
C1_BINS = [7, 1, 2, 3, 4, 5]
J_CHURN = 1080


def _random_codes(n, bins, C, seed=0, missing=0.0, device="cpu"):
    g = torch.Generator(device=device).manual_seed(seed)
    ld = max(16, (n + 15) // 16 * 16)
    codes = torch.full((len(bins), ld), 255, dtype=torch.uint8, device=device)
    for k, b in enumerate(bins):
        v = torch.randint(0, b, (n,), generator=g, device=device)
        v[torch.rand(n, generator=g, device=device) < missing] = 255
        codes[k, :n] = v.to(torch.uint8)
    labels = torch.full((ld,), 255, dtype=torch.uint8, device=device)
    lab = torch.randint(0, C, (n,), generator=g, device=device)
    lab[torch.rand(n, generator=g, device=device) < missing] = 255
    labels[:n] = lab.to(torch.uint8)
    return codes, labels


def _churn_probs():
    """float64 [1080]: probability of every joint state of the churn generator (class digit least
    significant, then feature 0, 1, ... as ``radix_layout``)."""
    p = torch.zeros(J_CHURN, dtype=torch.float64)
    for code in range(J_CHURN):
        c, rest = code % 2, code // 2
        pr, risk = 1.0, 25.0
        for (w, mult), r in zip(_CHURN_W, CHURN):
            k, rest = rest % r, rest // r
            pr *= w[k] / sum(w)
            risk *= mult[k]
        closed = min(risk, 99.0) / 100.0
        p[code] = pr * (closed if c == 1 else 1.0 - closed)
    return p


def _codes_of(rp):
    return H._radix_codes(rp, rp.words[:rp.n])


def _round_trip(code, J, b, counts=None):
    n = code.numel()
    sc, cs = H.patch_tables(torch.bincount(code, minlength=J) if counts is None else counts, b)
    stream, ei, ec = H.ref_patch_encode(code, sc, b)
    assert stream.dtype == torch.int32 and stream.numel() == (n + 31) // 32 * b
    assert ei.numel() == ec.numel() and bool((ec.long() > (1 << b) - 1).all())
    assert torch.equal(H.ref_patch_decode(stream, n, b, ei, ec, cs), code)
    return stream, ei, ec


# ---- CPU -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 31, 32, 33, 1001])
def test_twin_round_trip(n):
    g = torch.Generator().manual_seed(n)
    # churn-shaped skew
    code = torch.multinomial(_churn_probs(), n, replacement=True, generator=g)
    _round_trip(code, J_CHURN, 10)
    # uniform states; ranked from equal counts, b = 9 stores 511 of 1080 states: half the records escape
    code = torch.randint(0, J_CHURN, (n,), generator=g)
    _round_trip(code, J_CHURN, 10)
    _, ei, _ = _round_trip(code, J_CHURN, 9, counts=torch.ones(J_CHURN, dtype=torch.long))
    assert ei.numel() == int((code >= 511).sum())
    if n == 1001:
        assert 0.4 * n < ei.numel() < 0.65 * n
    # one state only
    _, ei, _ = _round_trip(torch.full((n,), 777), J_CHURN, 4)
    assert ei.numel() == 0
    # C = 1
    codes, _ = _random_codes(n, C1_BINS, 1, seed=n)
    rp = H.pack_rows(codes, n, C1_BINS, None, 1)
    assert rp.patched is None and rp.radices == C1_BINS          # CPU tensors never get a patched stream
    _round_trip(_codes_of(rp), 840, 9)
    # missing and unknown digits
    codes, labels = _random_codes(n, CHURN, 2, seed=n + 1, missing=0.3)
    rp = H.pack_rows(codes, n, CHURN, labels, 2)
    J = rp.class_radix * math.prod(rp.radices)
    for b in range(4, max(0, J - 1).bit_length()):
        _round_trip(_codes_of(rp), J, b)


def test_rank_tables():
    counts = torch.tensor([5, 9, 5, 0, 9, 1, 0, 7] + [0] * 12 + [3] * 12)     # J = 32, B = 5
    rank = H.patch_ranks(counts)
    J = counts.numel()
    assert sorted(rank.tolist()) == list(range(J))                            # a permutation
    by_rank = torch.argsort(rank)
    assert by_rank[:5].tolist() == [1, 4, 7, 0, 2]                            # ties: the smaller code first
    assert by_rank[5:17].tolist() == list(range(20, 32)) and by_rank[17].item() == 5
    assert by_rank[18:].tolist() == [3, 6] + list(range(8, 20))
    sc, cs = H.patch_tables(counts, 4)
    esc = 15
    assert sc.dtype == cs.dtype == torch.int16 and sc.numel() == J and cs.numel() == J + 1
    assert esc not in sc.tolist() and int(cs[esc]) == -1                      # ESC maps to nothing
    assert sorted(sc.tolist()) == [c for c in range(J + 1) if c != esc]
    assert torch.equal(cs.long()[sc.long()], torch.arange(J))                 # cell_state inverts state_cell
    assert torch.equal(sc.long(), torch.where(rank < esc, rank, rank + 1))
    for bad in (3, 5, 15):
        with pytest.raises(ValueError):
            H.patch_tables(counts, bad)


def test_choice_of_width():
    churn = (_churn_probs() * (1 << 40)).round().long()
    assert int((churn > 0).sum()) == 864
    assert H.choose_patch_bits(churn) == 10
    assert H.patch_cost(churn, 10) < 10 / 8 + 1e-6 < H.patch_cost(churn, 9)
    uniform = torch.full((J_CHURN,), 1000)
    assert H.choose_patch_bits(uniform, margin=0.9) is None
    assert H.choose_patch_bits(uniform, margin=1.0) == 10                     # 1.25 + 2 * 57 / 1080 < 1.375
    assert H.choose_patch_bits(torch.full((16,), 7)) is None                  # B = 4: no width below it
    assert H.choose_patch_bits(torch.zeros(J_CHURN, dtype=torch.long)) is None
    assert H.choose_patch_bits(torch.ones(1 << 15, dtype=torch.long)) is None  # J + 1 cells exceed 2^15


def test_misleading_sample_ends_without_stream():
    """First half one state, second half uniform, ranked from the head alone: the sample promises 4
    bits and no exceptions, the exact count after packing rejects the stream."""
    g = torch.Generator().manual_seed(5)
    n = 4096
    code = torch.cat([torch.full((n // 2,), 321), torch.randint(0, J_CHURN, (n // 2,), generator=g)])
    head = torch.bincount(code[:n // 2], minlength=J_CHURN)
    b = H.choose_patch_bits(head)
    assert b == 4 and H.patch_cost(head, b) == 0.5
    sc, cs = H.patch_tables(head, b)
    stream, ei, ec = H.ref_patch_encode(code, sc, b)
    assert torch.equal(H.ref_patch_decode(stream, n, b, ei, ec, cs), code)     # still lossless
    assert ei.numel() > 0.95 * (n // 2)
    assert not H.patch_keep(b, 11, n, ei.numel())
    assert H.patch_keep(b, 11, n, 0) and H.patch_keep(10, 11, n, 0) and not H.patch_keep(10, 11, n, n // 16)


# ---- GPU -----------------------------------------------------------------------------------------
def _churn_noise(n, seed):
    """Churn records with 0.1 % of them replaced by uniform ones (states the generator never emits)."""
    codes, labels = churn_device(n, seed=seed, device="cuda")
    g = torch.Generator(device="cuda").manual_seed(seed + 1)
    hit = torch.rand(n, generator=g, device="cuda") < 1e-3
    for k, b in enumerate(CHURN):
        v = torch.randint(0, b, (n,), generator=g, device="cuda").to(torch.uint8)
        codes[k, :n] = torch.where(hit, v, codes[k, :n])
    return codes, labels


def _make(kind, n):
    """(codes, labels or None, bins, C, RowPacked with the patched stream of the case)."""
    if kind == "churn_noise":
        codes, labels = _churn_noise(n, seed=n)
        rp = H.pack_rows(codes, n, CHURN, labels, 2)
        return codes, labels, CHURN, 2, rp
    if kind == "uniform_b9":
        codes, labels = _random_codes(n, CHURN, 2, seed=n, device="cuda")
        rp = H.attach_patched(H.pack_rows(codes, n, CHURN, labels, 2), bits=9)
        return codes, labels, CHURN, 2, rp
    if kind == "identical":
        codes = torch.tensor([2, 1, 0, 2, 4], dtype=torch.uint8, device="cuda").view(-1, 1).repeat(1, n)
        labels = torch.ones(n, dtype=torch.uint8, device="cuda")
        rp = H.pack_rows(codes, n, CHURN, labels, 2)
        return codes, labels, CHURN, 2, rp
    if kind == "c1":
        codes, _ = _random_codes(n, C1_BINS, 1, seed=n, device="cuda")
        rp = H.attach_patched(H.pack_rows(codes, n, C1_BINS, None, 1), bits=9)
        return codes, None, C1_BINS, 1, rp
    assert kind == "missing"
    codes, labels = _random_codes(n, CHURN, 2, seed=n, missing=0.05, device="cuda")
    rp = H.pack_rows(codes, n, CHURN, labels, 2)
    if rp.class_radix == 3 and rp.bits == 13:
        H.attach_patched(rp, bits=12)
    return codes, labels, CHURN, 2, rp


@gpu
@pytest.mark.parametrize("n", [1, 31, 32, 33, 4097])
@pytest.mark.parametrize("b", [9, 4])
def test_packer_equals_twin(n, b):
    codes, labels = _random_codes(n, CHURN, 2, seed=200 + n)
    rp_cpu = H.pack_rows(codes, n, CHURN, labels, 2)
    rp = H.attach_patched(H.pack_rows(codes.cuda(), n, CHURN, labels.cuda(), 2), bits=b)
    code = _codes_of(rp_cpu)
    assert rp.patched_bits == b and rp.bits == 11
    sc, cs = H.patch_tables(torch.bincount(code, minlength=J_CHURN), b)       # n <= 2^20: the sample is every record
    stream, ei, ec = H.ref_patch_encode(code, sc, b)
    assert torch.equal(rp.state_cell.cpu(), sc) and torch.equal(rp.cell_state.cpu(), cs)
    got = rp.patched.cpu()
    assert got.numel() == (n + 31) // 32 * b and torch.equal(got, stream)
    assert torch.equal(rp.exc_index.cpu(), ei) and torch.equal(rp.exc_cell.cpu(), ec)
    assert ei.numel() > 0 or n == 1 or (b == 9 and n < 512)     # fewer records than stored states: none escapes
    assert torch.equal(H.ref_patch_decode(got, n, b, rp.exc_index, rp.exc_cell, rp.cell_state), code)
    # padding records of the last group are zero bits
    last = got[-b:].long() & 0xFFFFFFFF
    used = (n - (n - 1) // 32 * 32) * b
    for i in range(b):
        assert int(last[i]) >> min(32, max(0, used - 32 * i)) == 0


def _check_counts(monkeypatch, codes, labels, bins, C, rp, n):
    ref = H.class_histogram(codes, n, bins, labels, C, count_labels=True).cpu()
    monkeypatch.delenv("AVMI_ROWPACK_KERNEL", raising=False)
    for r in (1, 32):
        monkeypatch.setenv("AVMI_JOINT_REPLICAS", str(r))
        assert torch.equal(H.class_histogram_packed(rp, count_labels=True).cpu(), ref), r
        assert torch.equal(H.class_histogram_packed(rp, count_labels=False).cpu(), ref[:, :-1]), r
        out = ref.cuda().clone()
        H.class_histogram_packed(rp, out=out, count_labels=True)
        assert torch.equal(out.cpu(), 2 * ref), r
    monkeypatch.delenv("AVMI_JOINT_REPLICAS")
    return ref


@gpu
@pytest.mark.parametrize("n", [1, 7, 2047, 2048, 2049, 3 * 2048 + 5, (1 << 20) + 13])
@pytest.mark.parametrize("kind", ["churn_noise", "uniform_b9", "identical", "c1", "missing"])
def test_patched_counts_equal_columns(monkeypatch, kind, n):
    """churn_noise asserts b = 10 and E > 0 at 2^20 + 13 records only: a sample of at most 6149 records
    holds too few distinct states for the rule to pick 10 bits, and one record cannot escape."""
    codes, labels, bins, C, rp = _make(kind, n)
    assert rp.patched is not None and rp.dense_is_radix and rp.patched_bits < rp.bits
    assert rp.patched.numel() == (n + 31) // 32 * rp.patched_bits and rp.dense.numel() == (n + 31) // 32 * rp.bits
    E = rp.exc_index.numel()
    if kind == "churn_noise" and n > 1 << 20:
        assert rp.patched_bits == 10 and E > 0
    if kind == "uniform_b9" and n >= 2047:          # 511 of 1080 states stored; a small sample ranks its own noise
        assert (0.4 if n > 1 << 20 else 0.1) * n < E < 0.65 * n
    if kind == "identical":
        assert rp.patched_bits == 4 and E == 0
    if kind == "missing" and n >= 2047:
        assert rp.class_radix == 3 and rp.patched_bits == 12 and (E > 0 or n < 1 << 20)   # 4095 states are stored
    _check_counts(monkeypatch, codes, labels, bins, C, rp, n)


@gpu
def test_misleading_sample_on_device(monkeypatch):
    """The packer's own count of escaped records rejects the stream a head sample asked for; the
    records are then counted from the plain stream."""
    n = 4096
    codes, labels = _random_codes(n, CHURN, 2, seed=9, device="cuda")
    codes[:, :n // 2] = torch.tensor([2, 1, 0, 2, 4], dtype=torch.uint8, device="cuda").view(-1, 1)
    labels[:n // 2] = 1
    rp = H.pack_rows(codes, n, CHURN, labels, 2)
    H.attach_patched(rp, sample=torch.arange(n // 2, device="cuda"))
    assert rp.patched is None and rp.patched_bits is None and rp.exc_index is None and rp.bits == 11
    monkeypatch.delenv("AVMI_ROWPACK_KERNEL", raising=False)
    ref = H.class_histogram(codes, n, CHURN, labels, 2, count_labels=True).cpu()
    assert torch.equal(H.class_histogram_packed(rp, count_labels=True).cpu(), ref)


@gpu
def test_identical_records_2_20(monkeypatch):
    n = 1 << 20
    codes, labels, bins, C, rp = _make("identical", n)
    assert rp.patched_bits == 4 and rp.exc_index.numel() == 0
    _check_counts(monkeypatch, codes, labels, bins, C, rp, n)


@gpu
def test_grid_stride_and_exception_loops_run_twice(monkeypatch):
    """More than 1024 * 256 groups of 32 records and more than 1024 * 256 exceptions."""
    n = (1 << 23) + (1 << 20) + 5
    codes, labels, bins, C, rp = _make("uniform_b9", n)
    assert rp.exc_index.numel() > 1 << 20
    assert bool((rp.exc_index[1:] > rp.exc_index[:-1]).all())
    _check_counts(monkeypatch, codes, labels, bins, C, rp, n)


@gpu
def test_other_kernels_on_the_same_records(monkeypatch):
    monkeypatch.delenv("AVMI_JOINT_REPLICAS", raising=False)
    n = 3 * 2048 + 5
    codes, labels, bins, C, rp = _make("churn_noise", n)
    assert rp.patched is not None
    ref = H.class_histogram(codes, n, bins, labels, C, count_labels=True).cpu()
    for kind in ("dense", "radix", "bitfield", "joint", "nibble"):
        monkeypatch.setenv("AVMI_ROWPACK_KERNEL", kind)
        assert torch.equal(H.class_histogram_packed(rp, count_labels=True).cpu(), ref), kind


@gpu
def test_bayes_patched_equals_columns(monkeypatch):
    monkeypatch.delenv("AVMI_JOINT_REPLICAS", raising=False)
    monkeypatch.delenv("AVMI_ROWPACK_KERNEL", raising=False)
    schema = FeatureSchema.from_json(CHURN_SCHEMA)
    n = (1 << 22) + 5
    codes, labels = churn_device(n, seed=11, device="cuda")
    t = Table(schema, n, codes, schema.feature_fields, torch.zeros((0, codes.shape[1]), device="cuda"), [],
              labels, schema.find_class_attr_field())
    a = NaiveBayes(schema).fit(t)
    t.pack_rows()
    assert t.rowpack.bits == 11 and t.rowpack.patched_bits == 10 and t.rowpack.patched is not None
    b = NaiveBayes(schema).fit(t)
    assert torch.equal(a.counts.cpu(), b.counts.cpu()) and torch.equal(a.class_n.cpu(), b.class_n.cpu())


@gpu
def test_bad_arguments_raise_before_launch():
    n = 4097
    codes, labels, bins, C, rp = _make("uniform_b9", n)
    out = torch.zeros((2, 19), dtype=torch.int64, device="cuda")
    offs = [0, 4, 7, 10, 13]

    def call(stream=rp.patched, b=9, exc=rp.exc_cell, cs=rp.cell_state):
        _native.C().class_histogram_patched(stream, n, b, list(rp.radices), list(rp.bins), offs, 2, 19, 2, out, True,
                                            exc, cs)

    for kw in (dict(b=3), dict(b=11), dict(cs=rp.cell_state[:-1].contiguous()), dict(stream=rp.patched[:-1].contiguous()),
               dict(cs=rp.cell_state.cpu())):
        with pytest.raises(RuntimeError):
            call(**kw)
    assert int(out.abs().sum()) == 0
    call()
    assert torch.equal(out.cpu(), H.class_histogram(codes, n, bins, labels, C, count_labels=True).cpu())
