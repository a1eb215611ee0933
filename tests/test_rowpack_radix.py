"""Mixed-radix record stream of the row-packed class histogram: layout numbers (joint states J,
bits per record B, table replicas R), a lossless torch reference of the code and of the dense
B-bit container, the HIP packer equal to that reference bit for bit, and the joint-table kernel's
counts equal to the byte-per-code column histogram ``H.class_histogram`` (the oracle of every
count here) over sizes around the group / block / grid boundaries, both class counts, missing
codes and unknown classes, and every replica count."""
import pytest
import torch

from avenir_amd.data.synth import CHURN_SCHEMA, churn_device
from avenir_amd.data.table import Table
from avenir_amd.models.bayes import NaiveBayes
from avenir_amd.ops import histogram as H
from avenir_amd.utils.schema import FeatureSchema

gpu = pytest.mark.gpu

CHURN = [4, 3, 3, 3, 5]


def _random_codes(n, bins, C, seed=0, missing=0.05, device="cpu"):
    g = torch.Generator(device=device).manual_seed(seed)
    F = len(bins)
    ld = max(16, (n + 15) // 16 * 16)
    codes = torch.full((F, ld), 255, dtype=torch.uint8, device=device)
    for k, b in enumerate(bins):
        v = torch.randint(0, b, (n,), generator=g, device=device)
        v[torch.rand(n, generator=g, device=device) < missing] = 255
        codes[k, :n] = v.to(torch.uint8)
    labels = torch.full((ld,), 255, dtype=torch.uint8, device=device)
    lab = torch.randint(0, C, (n,), generator=g, device=device)
    lab[torch.rand(n, generator=g, device=device) < missing] = 255
    labels[:n] = lab.to(torch.uint8)
    return codes, labels


# ---- torch reference of the code and of the container ------------------------------------------
def ref_encode(rp):
    """int64 [n] mixed-radix codes of the records of ``rp``, from ``unpack_rows``."""
    codes, labels = H.unpack_rows(rp)
    n = rp.n
    code = torch.zeros(n, dtype=torch.int64)
    mult = 1
    if rp.class_radix > 1:
        lab = labels[:n].long().cpu()
        code += torch.where(lab < rp.n_classes, lab, torch.full_like(lab, 2))
        mult = rp.class_radix
    for k, (b, r) in enumerate(zip(rp.bins, rp.radices)):
        v = codes[k, :n].long().cpu()
        code += torch.where(v < b, v, torch.full_like(v, b)) * mult
        mult *= r
    assert int(code.max()) < mult
    return code


def ref_decode(rp, code):
    """(codes uint8 [F, n], labels uint8 [n] or None) with 255 for missing / unknown."""
    code = code.clone()
    labels = None
    if rp.class_radix > 1:
        c = code % rp.class_radix
        code //= rp.class_radix
        labels = torch.where(c < rp.n_classes, c, torch.full_like(c, 255)).to(torch.uint8)
    out = []
    for b, r in zip(rp.bins, rp.radices):
        v = code % r
        code //= r
        out.append(torch.where(v < b, v, torch.full_like(v, 255)).to(torch.uint8))
    assert int(code.max()) == 0
    return torch.stack(out), labels


def ref_pack_bits(code, B):
    """int32 [ceil(n / 32) * B]: record k of group g at bits [k B, k B + B) of the group's B dwords."""
    n = code.numel()
    r = torch.arange(n)
    pos = (r // 32) * (32 * B) + (r % 32) * B
    acc = torch.zeros((n + 31) // 32 * B, dtype=torch.int64)
    for b in range(B):
        acc.index_add_(0, (pos + b) // 32, ((code >> b) & 1) << ((pos + b) % 32))
    return torch.where(acc >= 1 << 31, acc - (1 << 32), acc).to(torch.int32)


def ref_unpack_bits(dense, n, B):
    d = dense.long() & 0xFFFFFFFF
    r = torch.arange(n)
    pos = (r // 32) * (32 * B) + (r % 32) * B
    code = torch.zeros(n, dtype=torch.int64)
    for b in range(B):
        code |= ((d[(pos + b) // 32] >> ((pos + b) % 32)) & 1) << b
    return code


# ---- CPU -----------------------------------------------------------------------------------------
def test_radix_layout_numbers(monkeypatch):
    monkeypatch.delenv("AVMI_JOINT_REPLICAS", raising=False)
    no = [False] * 5
    assert H.radix_layout(CHURN, 2, no, unknown=False) == ([4, 3, 3, 3, 5], 2, 1080, 11, 32)
    assert H.radix_layout(CHURN, 2, no, unknown=True) == ([4, 3, 3, 3, 5], 3, 1620, 11, 16)
    assert H.radix_layout(CHURN, 2, [True] * 5, unknown=True) == ([5, 4, 4, 4, 6], 3, 5760, 13, 4)
    assert H.radix_layout([8] * 5, 1, no) == ([8] * 5, 1, 32768, 15, 1)
    assert H.radix_layout([8] * 5 + [2], 1, [False] * 6) is None          # J = 2^16: no dense stream
    assert H.radix_layout([2, 2], 2, [False] * 2, unknown=False) is None  # J = 8: under 4 bits
    # the radix record never needs more bits than the bit-field record
    for bins, C, miss in [(CHURN, 2, no), (CHURN, 2, [True] * 5), ([7, 1, 2, 3, 4, 5], 1, [True] * 6)]:
        sh, wd, lsh, lw = H.rowpack_layout(bins, C, miss)
        lay = H.radix_layout(bins, C, miss, unknown=True)
        assert lay[3] <= max([s + w for s, w in zip(sh, wd)] + [lsh + lw]) and lay[2] <= 1 << lay[3]


def test_radix_replicas_env_is_clamped(monkeypatch):
    for want, got in [("1", 1), ("2", 2), ("3", 2), ("8", 8), ("64", 32), ("0", 1)]:
        monkeypatch.setenv("AVMI_JOINT_REPLICAS", want)
        assert H.radix_layout(CHURN, 2, [False] * 5, unknown=False)[4] == got
    monkeypatch.setenv("AVMI_JOINT_REPLICAS", "32")
    assert H.radix_layout(CHURN, 2, [True] * 5, unknown=True)[4] == 4      # what fits, not what was asked


@pytest.mark.parametrize("C,missing", [(2, 0.05), (2, 0.0), (1, 0.05)])
def test_radix_code_round_trip(C, missing):
    bins = CHURN if C == 2 else [7, 1, 2, 3, 4, 5]
    n = 1001
    codes, labels = _random_codes(n, bins, C, seed=3, missing=missing)
    rp = H.pack_rows(codes, n, bins, labels if C == 2 else None, C)
    assert rp.radices == [b + (1 if missing else 0) for b in bins]
    assert rp.class_radix == (1 if C == 1 else (3 if missing else 2))
    _, _, J, B, _ = H.radix_layout(bins, C, [missing > 0] * len(bins), unknown=missing > 0)
    code = ref_encode(rp)
    assert int(code.max()) < J
    dense = ref_pack_bits(code, B)
    assert dense.numel() == (n + 31) // 32 * B
    back = ref_unpack_bits(dense, n, B)
    assert torch.equal(back, code)
    c2, l2 = ref_decode(rp, back)
    c1, l1 = H.unpack_rows(rp)
    assert torch.equal(c1[:, :n], c2)
    if C == 2:
        assert torch.equal(l1[:n], l2)


# ---- GPU -----------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("n", [1, 31, 32, 33, 4097])
@pytest.mark.parametrize("missing", [0.0, 0.05])
def test_pack_radix_stream_equals_reference(n, missing):
    codes, labels = _random_codes(n, CHURN, 2, seed=100 + n, missing=missing)
    rp_cpu = H.pack_rows(codes, n, CHURN, labels, 2)
    rp = H.pack_rows(codes.cuda(), n, CHURN, labels.cuda(), 2)
    assert rp.dense_is_radix and rp.radices == rp_cpu.radices and rp.class_radix == rp_cpu.class_radix
    B = rp.bits
    assert B == H.radix_layout(CHURN, 2, [r > b for r, b in zip(rp.radices, CHURN)], rp.class_radix == 3)[3]
    ref = ref_pack_bits(ref_encode(rp_cpu), B)
    got = rp.dense.cpu()
    assert got.numel() == (n + 31) // 32 * B == ref.numel()
    assert torch.equal(got, ref)
    # padding records of the last group are zero bits
    last = got[-B:].long() & 0xFFFFFFFF
    used = (n - (n - 1) // 32 * 32) * B
    for i in range(B):
        keep = min(32, max(0, used - 32 * i))
        assert int(last[i]) >> keep == 0


@gpu
@pytest.mark.parametrize("n", [1, 7, 32, 63, 4097, (1 << 20) + 13, (1 << 23) + (1 << 20) + 5])
@pytest.mark.parametrize("C", [1, 2])
@pytest.mark.parametrize("missing", [0.0, 0.05])
def test_radix_counts_equal_columns(monkeypatch, n, C, missing):
    """The largest n has more than 1024 * 256 groups of 32 records: the grid-stride loop runs twice."""
    bins = CHURN if C == 2 else [7, 1, 2, 3, 4, 5]
    codes, labels = _random_codes(n, bins, C, seed=n, missing=missing, device="cuda")
    lab = labels if C == 2 else None
    ref = H.class_histogram(codes, n, bins, lab, C, count_labels=True).cpu()
    monkeypatch.delenv("AVMI_ROWPACK_KERNEL", raising=False)
    rp = H.pack_rows(codes, n, bins, lab, C)
    assert rp is not None and rp.dense_is_radix and rp.dense.numel() == (n + 31) // 32 * rp.bits
    for r in (1, 2, 4, 8, 16, 32):
        monkeypatch.setenv("AVMI_JOINT_REPLICAS", str(r))
        got = H.class_histogram_packed(rp, count_labels=True).cpu()
        assert torch.equal(got, ref), r
    monkeypatch.delenv("AVMI_JOINT_REPLICAS")
    assert torch.equal(H.class_histogram_packed(rp, count_labels=False).cpu(), ref[:, :-1])
    # accumulates into a given table, as partial_fit uses it
    out = ref.cuda().clone()
    H.class_histogram_packed(rp, out=out, count_labels=True)
    assert torch.equal(out.cpu(), 2 * ref)
    # the bit-field stream of the same records stays reachable
    monkeypatch.setenv("AVMI_ROWPACK_KERNEL", "bitfield")
    assert torch.equal(H.class_histogram_packed(rp, count_labels=True).cpu(), ref)


@gpu
def test_radix_single_replica_15_bits_and_too_many_states(monkeypatch):
    monkeypatch.delenv("AVMI_JOINT_REPLICAS", raising=False)
    monkeypatch.delenv("AVMI_ROWPACK_KERNEL", raising=False)
    n = 100003
    bins = [8] * 5
    codes, _ = _random_codes(n, bins, 1, seed=5, missing=0.0, device="cuda")
    ref = H.class_histogram(codes, n, bins, None, 1, count_labels=True).cpu()
    rp = H.pack_rows(codes, n, bins, None, 1)
    assert rp.dense_is_radix and rp.bits == 15 and H.radix_layout(bins, 1, [False] * 5)[4] == 1
    assert torch.equal(H.class_histogram_packed(rp, count_labels=True).cpu(), ref)
    # J = 2^16 states: no dense stream, the 16-bit words are counted
    bins = [8] * 5 + [2]
    codes, _ = _random_codes(n, bins, 1, seed=6, missing=0.0, device="cuda")
    rp = H.pack_rows(codes, n, bins, None, 1)
    assert rp is not None and rp.dense is None and not rp.dense_is_radix
    ref = H.class_histogram(codes, n, bins, None, 1, count_labels=True).cpu()
    assert torch.equal(H.class_histogram_packed(rp, count_labels=True).cpu(), ref)


@gpu
def test_radix_uniform_run(monkeypatch):
    """2^24 identical records: every lane adds to one cell (same-address atomics within a replica),
    and the count is spread over all replicas, which the rotated replica sum must collect."""
    monkeypatch.delenv("AVMI_JOINT_REPLICAS", raising=False)
    monkeypatch.delenv("AVMI_ROWPACK_KERNEL", raising=False)
    n = 1 << 24
    vals = [2, 1, 0, 2, 4]
    codes = torch.tensor(vals, dtype=torch.uint8, device="cuda").view(-1, 1).repeat(1, n)
    labels = torch.ones(n, dtype=torch.uint8, device="cuda")
    rp = H.pack_rows(codes, n, CHURN, labels, 2)
    assert rp.dense_is_radix and rp.bits == 11 and rp.class_radix == 2
    got = H.class_histogram_packed(rp, count_labels=True).cpu()
    exp = torch.zeros_like(got)
    for o, v in zip([0, 4, 7, 10, 13], vals):
        exp[1, o + v] = n
    exp[1, -1] = n
    assert torch.equal(got, exp)


@gpu
def test_bayes_radix_packed_equals_columns(monkeypatch):
    monkeypatch.delenv("AVMI_JOINT_REPLICAS", raising=False)
    monkeypatch.delenv("AVMI_ROWPACK_KERNEL", raising=False)
    schema = FeatureSchema.from_json(CHURN_SCHEMA)
    n = (1 << 22) + 5
    codes, labels = churn_device(n, seed=11, device="cuda")
    t = Table(schema, n, codes, schema.feature_fields, torch.zeros((0, codes.shape[1]), device="cuda"), [],
              labels, schema.find_class_attr_field())
    a = NaiveBayes(schema).fit(t)
    t.pack_rows()
    assert t.rowpack is not None and t.rowpack.dense_is_radix and t.rowpack.bits == 11
    b = NaiveBayes(schema).fit(t)
    assert torch.equal(a.counts.cpu(), b.counts.cpu()) and torch.equal(a.class_n.cpu(), b.class_n.cpu())
