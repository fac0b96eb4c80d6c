"""GPU: the caller-stream contract of every entry point that takes device buffers (include/h2agg.h: h2agg_set_stream; "queued
on the context's stream, no synchronisation").  tests/stream_probe.py has the method: the context is on a torch stream s, s is
held busy, the true input reaches the input buffer only behind the hold, and until then the buffer holds a decoy — a second
valid input with another result.  Whatever the library runs off s, or reads before the hold ends, computes the decoy's
result.

CASES names every h2agg_*_device / *_async declaration of the header (tests/test_stream_probe_host.py holds the two sets
against each other) as `queued` or `synchronous`; every case has one or more variants, each a Work built from the suite's
references alone: tests/quotient_ref.py, grand_product_ref.py, lookup_permute_ref.py, poly_open_ref.py, oracle.bn254, and
Python integers for the transform.  Every comparison is byte for byte (Jacobian results as affine points: include/h2agg.h)."""
import functools
import importlib
import random
import time

import numpy as np
import pytest
import torch

import __graft_entry__ as entry
from oracle import bn254 as O
from tests import grand_product_ref as G
from tests import poly_open_ref as PO
from tests import quotient_ref as Q
from tests import stream_probe as SP
from tests.fr_bytes import enc, fe
from tests.lookup_permute_ref import compress_py, lookup_permute_py

pytestmark = pytest.mark.gpu

R = O.R
K = 9                      # the Fr shapes: 512 rows, several workgroups
N = 1 << K
U = N - 6                  # usable rows with five blinding rows
QK = 4                     # the key of the expression and quotient cases
MSM_SIZES = (3000, (1 << 15) + 5, (1 << 16) + 5)   # one-launch sort, packed two-level sort, digit-major sort with 16-bit windows
MSM_TABLE = max(MSM_SIZES)
KZG_TAU = 0x5EC12E7F00D


def slab(columns):
    return b"".join(enc(c) for c in columns)


def image(total, *parts):
    """what d_out must hold behind a call: PATTERN everywhere but the (offset, bytes) the call writes"""
    out = bytearray([SP.PATTERN]) * total
    for at, data in parts:
        out[at:at + len(data)] = data
    return bytes(out)


def affine(jac: bytes) -> bytes:
    """canonical Jacobian points -> canonical affine, with Python integers"""
    return b"".join(O.aff_to_bytes(O.jac_from_bytes(jac[i:i + 96])) for i in range(0, len(jac), 96))


def fr_column(seed, n=N):
    """random canonical elements with 0, 1 and r - 1 among them"""
    rng = random.Random(seed)
    a = [rng.randrange(R) for _ in range(n)]
    for pos, v in zip(rng.sample(range(n), 3), (R - 1, 0, 1)):
        a[pos] = v
    return a


def nonzero_column(seed, n=N):
    rng = random.Random(seed)
    return [rng.randrange(1, R) for _ in range(n)]


@functools.lru_cache(maxsize=None)
def msm_scalars(seed, n):
    """-> (values, their 32-byte encodings back to back)"""
    raw = np.random.Generator(np.random.PCG64(seed)).bytes(64 * n)
    vals = [int.from_bytes(raw[64 * i:64 * i + 64], "little") % R for i in range(n)]
    return vals, b"".join(v.to_bytes(32, "little") for v in vals)


def msm_point(ks, ss, n):
    """(sum_{i<n} k_i s_i) G as canonical affine bytes"""
    return O.aff_to_bytes(O.scalar_mul(sum(k * s for k, s in zip(ks[:n], ss[:n])) % R, O.G1))


class Work:
    """One variant of one case: the true and the decoy input (the bytes of one input buffer), what the output buffer must
    hold behind a call on each, and how the call is made.  call(ctx, res, d_in, d_out) queues (or, for a synchronous entry
    point, makes and returns) the library call on pointers into the two buffers; res is the context's Resources."""

    def __init__(self, true_in, decoy_in, want, want_decoy, call, out_bytes=0, in_place=False, view=None, warm=1):
        self.true_in, self.decoy_in, self.want, self.want_decoy = true_in, decoy_in, want, want_decoy
        self.call, self.out_bytes, self.in_place, self.view, self.warm = call, out_bytes, in_place, view or (lambda b: b), warm
        self.raw = view is None            # want is the image of the whole output buffer
        assert len(true_in) == len(decoy_in)


# ---------------------------------------------------------------------------------------------- the Fr transform
@functools.lru_cache(maxsize=None)
def work_fft(in_place):
    a, d = fr_column(0xA001), fr_column(0xA002)
    inverse, shift = (True, None) if in_place else (False, Q.ZETA)
    ref = lambda x: enc(Q.ntt(x, K, shift or 1, inverse))
    sh = None if shift is None else fe(shift)

    def call(ctx, res, d_in, d_out):
        ctx.fr_fft_device(d_in, K, inverse, sh, d_in if in_place else d_out)
    return Work(enc(a), enc(d), ref(a), ref(d), call, 32 * N, in_place)


# ---------------------------------------------------------------------------------------------- KZG openings
@functools.lru_cache(maxsize=None)
def work_divide(in_place):
    a, d, z = fr_column(0xA011), fr_column(0xA012), PO.BIG_Z
    if in_place:
        ref = lambda x: enc(PO.quotient_py(x, z))
        call = lambda ctx, res, d_in, d_out: ctx.fr_poly_divide_device(d_in, K, fe(z), d_in, None)
        return Work(enc(a), enc(d), ref(a), ref(d), call, 32 * N, True)
    ref = lambda x: enc(PO.quotient_py(x, z)) + fe(PO.horner(x, z))
    call = lambda ctx, res, d_in, d_out: ctx.fr_poly_divide_device(d_in, K, fe(z), d_out, d_out + 32 * N)
    return Work(enc(a), enc(d), ref(a), ref(d), call, 32 * N + 32)


EVAL_QUERIES = [(1, 0), (0, 1), (1, 1), (0, 0)]


@functools.lru_cache(maxsize=None)
def work_poly_eval():
    zs = [PO.BIG_Z, 0x1234567]
    polys = lambda seed: [fr_column(seed), fr_column(seed + 1)]
    ref = lambda ps: enc([PO.horner(ps[m], zs[p]) for m, p in EVAL_QUERIES])
    a, d = polys(0xA021), polys(0xA031)
    call = lambda ctx, res, d_in, d_out: ctx.fr_poly_eval_device(d_in, 2, K, EVAL_QUERIES, enc(zs))
    return Work(slab(a), slab(d), ref(a), ref(d), call)


MO_QUERIES = [(0, 1), (1, 0), (2, 1), (0, 0), (1, 1)]


def multiopen_ws(polys, zs, v):
    """W_g = ((sum_m v^m (p_m(tau) - p_m(z_g))) / (tau - z_g)) G per group of MO_QUERIES in first-seen order -> ([points], [W])"""
    groups = []
    for m, pt in MO_QUERIES:
        for g in groups:
            if g[0] == pt:
                g[1].append(m)
                break
        else:
            groups.append((pt, [m]))
    ws = []
    for pt, members in groups:
        acc, vm = 0, 1
        for m in members:
            acc = (acc + vm * (PO.horner(polys[m], KZG_TAU) - PO.horner(polys[m], zs[pt]))) % R
            vm = vm * v % R
        d = acc * O.inv((KZG_TAU - zs[pt]) % R, R) % R
        ws.append(O.aff_to_bytes(O.scalar_mul(d, O.G1)) if d else bytes(64))
    return [pt for pt, _m in groups], ws


@functools.lru_cache(maxsize=None)
def work_multiopen():
    zs, v = [0x7777, PO.BIG_Z], 0xABCDEF0123
    polys = lambda seed: [fr_column(seed + m) for m in range(3)]
    a, d = polys(0xA041), polys(0xA051)
    ref = lambda ps: b"".join(multiopen_ws(ps, zs, v)[1])

    def call(ctx, res, d_in, d_out):
        gp, ws = ctx.kzg_multiopen_device(res.kzg_g(), d_in, 3, K, MO_QUERIES, enc(zs), fe(v))
        assert gp == [1, 0], "the groups' points in first-seen order"
        return b"".join(ws)
    return Work(slab(a), slab(d), ref(a), ref(d), call)


# ---------------------------------------------------------------------------------------------- grand products
@functools.lru_cache(maxsize=None)
def work_batch_invert():
    a, d = fr_column(0xA061), fr_column(0xA062)
    ref = lambda x: enc(G.batch_invert_py(x))
    call = lambda ctx, res, d_in, d_out: ctx.fr_batch_invert_device(d_in, N, d_out)
    return Work(enc(a), enc(d), ref(a), ref(d), call, 32 * N)


def z_image(z):
    """d_out of a product call: z[0 .. U] in a column of N rows, then d_last"""
    return image(32 * N + 32, (0, enc(z)), (32 * N, fe(z[U])))


@functools.lru_cache(maxsize=None)
def work_grand_product():
    init = G.BIG
    pair = lambda seed: (fr_column(seed), nonzero_column(seed + 1))
    ref = lambda nd: z_image(G.grand_product_py(nd[0], nd[1], U, init))
    a, d = pair(0xA071), pair(0xA081)
    call = lambda ctx, res, d_in, d_out: ctx.fr_grand_product_device(d_in, d_in + 32 * N, K, U, fe(init), d_out, d_out + 32 * N)
    return Work(slab(a), slab(d), ref(a), ref(d), call, 32 * N + 32)


@functools.lru_cache(maxsize=None)
def work_permutation_product():
    m = 3
    rng = random.Random(0xA091)
    beta, gamma, init = rng.randrange(R), rng.randrange(R), rng.randrange(1, R)
    delta_first = pow(G.DELTA, 2, R)

    def build(seed):
        values, sigmas = G.satisfied_permutation(seed, K, m, U)
        _num, den = G.permutation_terms_py(values, sigmas, K, U, beta, gamma, G.DELTA, delta_first)
        assert all(den), "a zero denominator"
        return values, sigmas
    ref = lambda vs: z_image(G.permutation_product_py(vs[0], vs[1], K, U, beta, gamma, G.DELTA, delta_first, init))
    a, d = build(0xA092), build(0xA093)
    call = lambda ctx, res, d_in, d_out: ctx.permutation_product_device(
        d_in, d_in + 32 * N * m, m, K, U, fe(beta), fe(gamma), fe(G.DELTA), fe(delta_first), fe(init), d_out, d_out + 32 * N)
    return Work(slab(a[0] + a[1]), slab(d[0] + d[1]), ref(a), ref(d), call, 32 * N + 32)


@functools.lru_cache(maxsize=None)
def work_lookup_product():
    rng = random.Random(0xA0A1)
    beta, gamma = rng.randrange(R), rng.randrange(R)

    def build(seed):
        cols = G.permuted_pair(seed, K, U)
        assert all((cols[2][i] + beta) % R and (cols[3][i] + gamma) % R for i in range(U)), "a zero denominator"
        return cols
    ref = lambda c: z_image(G.lookup_product_py(c[0], c[1], c[2], c[3], U, beta, gamma))
    a, d = build(0xA0A2), build(0xA0A3)
    call = lambda ctx, res, d_in, d_out: ctx.lookup_product_device(
        d_in, d_in + 32 * N, d_in + 64 * N, d_in + 96 * N, K, U, fe(beta), fe(gamma), d_out, d_out + 32 * N)
    return Work(slab(a), slab(d), ref(a), ref(d), call, 32 * N + 32)


# ---------------------------------------------------------------------------------------------- lookup argument
@functools.lru_cache(maxsize=None)
def work_lookup_permute():
    def build(seed):
        a, s, _ap, _sp = G.permuted_pair(seed, K, U)
        assert set(a[:U]) <= set(s[:U]), "an input value that is not in the table"
        return a, s

    def ref(pair):
        ap, sp = lookup_permute_py(pair[0], pair[1], U)
        return image(64 * N, (0, enc(ap)), (32 * N, enc(sp)))       # the rows from U up are the caller's
    a, d = build(0xA0B1), build(0xA0B2)
    call = lambda ctx, res, d_in, d_out: ctx.lookup_permute_device(d_in, d_in + 32 * N, K, U, d_out, d_out + 32 * N)
    return Work(slab(a), slab(d), ref(a), ref(d), call, 64 * N)


@functools.lru_cache(maxsize=None)
def work_columns_compress():
    m, theta = 3, G.BIG
    cols = lambda seed: [fr_column(seed + j) for j in range(m)]
    ref = lambda c: enc(compress_py(c, theta))
    a, d = cols(0xA0C1), cols(0xA0D1)
    call = lambda ctx, res, d_in, d_out: ctx.fr_columns_compress_device(d_in, m, K, fe(theta), d_out)
    return Work(slab(a), slab(d), ref(a), ref(d), call, 32 * N)


# ---------------------------------------------------------------------------------------------- expressions, quotient
@functools.lru_cache(maxsize=None)
def quotient_key():
    """k = 4, degree 4 (e = 2, chunk_len 2), three permutation columns (two sets, the last ragged), one lookup, gates"""
    return Q.random_shape(random.Random(0xA0E1), QK, 4, 3, 1, True)


def slab_pointers(cs, kinds, base):
    """the slabs of `kinds` back to back from `base` on: a pointer per kind, None for a kind without columns"""
    counts = {"advice": cs.num_advice_columns, "fixed": len(cs.fixed_commitments), "instance": cs.num_instance_columns,
              "sigma": len(cs.permutation_columns), "perm_z": cs.num_permutation_sets, "lookup_z": len(cs.lookups),
              "lookup_ap": len(cs.lookups), "lookup_sp": len(cs.lookups)}
    out, at = [], base
    for kind in kinds:
        out.append(at if counts[kind] else None)
        at += 32 * cs.n * counts[kind]
    return out


@functools.lru_cache(maxsize=None)
def work_expressions(fold):
    """fold False: every gate polynomial as a column; True: the theta-fold of lookup 0's input expressions"""
    cs = quotient_key()
    theta = G.BIG
    which, th = (1, theta) if fold else (0, None)
    kinds = ("advice", "fixed", "instance")
    rows = lambda seed: Q.random_inputs(random.Random(seed), cs)

    def ref(p):
        out = Q.expressions_rows_py(cs, which, 0, p["advice"], p["fixed"], p["instance"], [], th)
        return enc(out) if fold else slab(out)
    a, d = rows(0xA0E2), rows(0xA0E3)
    out_bytes = 32 * cs.n * (1 if fold else len(Q.expression_lists(cs, 0)))

    def call(ctx, res, d_in, d_out):
        ctx.vk_expressions_eval_device(res.vk(cs), which, 0, cs.k, *slab_pointers(cs, kinds, d_in), None,
                                       None if th is None else fe(th), d_out)
    as_bytes = lambda p: b"".join(slab(p[kind]) for kind in kinds)
    return Work(as_bytes(a), as_bytes(d), ref(a), ref(d), call, out_bytes)


@functools.lru_cache(maxsize=None)
def work_quotient():
    cs = quotient_key()
    sc = Q.random_scalars(random.Random(0xA0F1))
    polys = lambda seed: Q.random_inputs(random.Random(seed), cs)
    ref = lambda p: slab(Q.quotient_py(cs, *Q.quotient_args(p, sc))[0])
    a, d = polys(0xA0F2), polys(0xA0F3)

    def call(ctx, res, d_in, d_out):
        ctx.quotient_device(res.vk(cs), *slab_pointers(cs, Q.POLY_KINDS, d_in), None, fe(sc["theta"]), fe(sc["beta"]),
                            fe(sc["gamma"]), fe(sc["y"]), fe(sc["delta"]), d_out)
    as_bytes = lambda p: b"".join(slab(p[kind]) for kind in Q.POLY_KINDS)
    return Work(as_bytes(a), as_bytes(d), ref(a), ref(d), call, 32 * cs.n * (cs.degree - 1))


# ---------------------------------------------------------------------------------------------- G1
def table_scalars():
    return msm_scalars(0xB001, MSM_TABLE)


@functools.lru_cache(maxsize=None)
def work_msm(n, batch):
    """batch 0: h2agg_g1_msm_device_async; batch 2: h2agg_g1_msm_device_batch_async over [2][n] scalars.  The decoy is a second
    set of scalars.  Three warm-up calls: one per tail slot of the context."""
    ks, _kb = table_scalars()
    sets = lambda seed: [msm_scalars(seed + q, n) for q in range(max(batch, 1))]
    ref = lambda ss: b"".join(msm_point(ks, vals, n) for vals, _b in ss)
    as_bytes = lambda ss: b"".join(b for _vals, b in ss)
    a, d = sets(0xB100 + n), sets(0xB200 + n)
    if batch:
        call = lambda ctx, res, d_in, d_out: ctx.g1_msm_device_batch_async(res.table(), d_in, n, batch, d_out)
    else:
        call = lambda ctx, res, d_in, d_out: ctx.g1_msm_device_async(res.table(), d_in, n, d_out)
    return Work(as_bytes(a), as_bytes(d), ref(a), ref(d), call, 96 * max(batch, 1), view=affine, warm=3)


@functools.lru_cache(maxsize=None)
def work_msm_sync():
    n = MSM_SIZES[0]
    ks, _kb = table_scalars()
    a, d = msm_scalars(0xB301, n), msm_scalars(0xB302, n)
    call = lambda ctx, res, d_in, d_out: affine(ctx.g1_msm_device(res.table(), d_in, n))
    return Work(a[1], d[1], msm_point(ks, a[0], n), msm_point(ks, d[0], n), call, warm=3)


@functools.lru_cache(maxsize=None)
def work_to_affine():
    """300 points i G in Jacobian form with a z of their own each"""
    n = 300

    def build(seed):
        rng = random.Random(seed)
        pts, p = [], O.scalar_mul(rng.randrange(R), O.G1)
        for _ in range(n):
            pts.append(p)
            p = O.add(p, O.G1)
        return pts, b"".join(O.jac_to_bytes(pt, rng.randrange(1, O.P)) for pt in pts)
    ref = lambda pts: b"".join(O.aff_to_bytes(pt) for pt in pts)
    a, d = build(0xB401), build(0xB402)
    call = lambda ctx, res, d_in, d_out: ctx.g1_batch_to_affine_device(d_in, n)
    return Work(a[1], d[1], ref(a[0]), ref(d[0]), call)


@functools.lru_cache(maxsize=None)
def work_bases_generate():
    """the table k_i G of scalars in device memory, seen through the MSM over it: (sum k_i s_i) G"""
    n = 300
    ss, sb = msm_scalars(0xB501, n)
    a, d = msm_scalars(0xB502, n), msm_scalars(0xB503, n)

    def call(ctx, res, d_in, d_out):
        handle = ctx.bases_generate(d_in, n)
        try:
            return affine(ctx.g1_msm_preloaded(handle, sb))
        finally:
            ctx.bases_free(handle)
    return Work(a[1], d[1], msm_point(a[0], ss, n), msm_point(d[0], ss, n), call)


# ---------------------------------------------------------------------------------------------- the case table
QUEUED, SYNCHRONOUS = "queued", "synchronous"
CASES = {
    "h2agg_fr_fft_device": (QUEUED, {"out_of_place_coset": lambda: work_fft(False), "in_place_inverse": lambda: work_fft(True)}),
    "h2agg_fr_poly_divide_device": (QUEUED, {"in_place": lambda: work_divide(True), "with_rem": lambda: work_divide(False)}),
    "h2agg_fr_batch_invert_device": (QUEUED, {"k9": work_batch_invert}),
    "h2agg_fr_grand_product_device": (QUEUED, {"k9": work_grand_product}),
    "h2agg_permutation_product_device": (QUEUED, {"k9": work_permutation_product}),
    "h2agg_lookup_product_device": (QUEUED, {"k9": work_lookup_product}),
    "h2agg_lookup_permute_device": (QUEUED, {"k9": work_lookup_permute}),
    "h2agg_fr_columns_compress_device": (QUEUED, {"k9": work_columns_compress}),
    "h2agg_vk_expressions_eval_device": (QUEUED, {"columns": lambda: work_expressions(False), "fold": lambda: work_expressions(True)}),
    "h2agg_quotient_device": (QUEUED, {"k4": work_quotient}),
    "h2agg_g1_msm_device_async": (QUEUED, {"n%d" % n: functools.partial(work_msm, n, 0) for n in MSM_SIZES}),
    "h2agg_g1_msm_device_batch_async": (QUEUED, {"n%d" % n: functools.partial(work_msm, n, 2) for n in MSM_SIZES}),
    "h2agg_g1_batch_to_affine_device": (SYNCHRONOUS, {"n300": work_to_affine}),
    "h2agg_g1_msm_device": (SYNCHRONOUS, {"n3000": work_msm_sync}),
    "h2agg_fr_poly_eval_device": (SYNCHRONOUS, {"k9": work_poly_eval}),
    "h2agg_kzg_multiopen_device": (SYNCHRONOUS, {"k9": work_multiopen}),
}
# reads device memory without saying so in its name: the header's pattern does not find it, the case is kept beside the table
EXTRA_SYNCHRONOUS = {"h2agg_bases_generate": {"n300": work_bases_generate}}

MSM_CASES = ("h2agg_g1_msm_device_async", "h2agg_g1_msm_device_batch_async")


def variants(kind, names=None):
    return [(name, v) for name, (k, vs) in CASES.items() if k == kind and (names is None or name in names) for v in vs]


def every_work():
    for name, (_kind, vs) in list(CASES.items()) + [(n, (SYNCHRONOUS, vs)) for n, vs in EXTRA_SYNCHRONOUS.items()]:
        for v, build in vs.items():
            yield name, v, build


# ---------------------------------------------------------------------------------------------- contexts
class Resources:
    """what the calls of one context need beside the two buffers: the MSM table, the KZG monomial table, the keys"""

    def __init__(self, pkg, ctx):
        self.ctx, self._table, self._g, self._vks = ctx, None, None, {}
        self._verifier = importlib.import_module(entry.PKG_NAME + ".verifier")

    def table(self):
        if self._table is None:
            d_k = SP.to_device(table_scalars()[1])
            self._table = self.ctx.bases_generate(d_k.data_ptr(), MSM_TABLE)
        return self._table

    def kzg_g(self):
        if self._g is None:
            self._g = self.ctx.params_setup(K, fe(KZG_TAU))
        return self._g[0]

    def vk(self, cs):
        if id(cs) not in self._vks:
            self._vks[id(cs)] = self._verifier.VerifyingKey(self.ctx, self._verifier.encode_vk(cs, O.aff_to_bytes))
        return self._vks[id(cs)]

    def close(self):
        for vk in self._vks.values():
            vk.close()
        for h in ([self._table] if self._table else []) + list(self._g or ()):
            self.ctx.bases_free(h)


class OnStream:
    """a context of its own on a torch stream of its own"""

    def __init__(self, pkg, stream=None):
        self.ctx = pkg.H2Agg(0)
        self.s = stream or torch.cuda.Stream()
        self.ctx.set_stream(self.s.cuda_stream)
        self.res = Resources(pkg, self.ctx)

    def close(self):
        self.res.close()
        self.ctx.close()


@pytest.fixture(scope="module")
def on_s(pkg):
    o = OnStream(pkg)
    yield o
    o.close()


def buffers(work):
    d_in = torch.zeros(len(work.true_in), dtype=torch.uint8, device=SP.device())
    d_out = d_in if work.in_place else torch.zeros(max(work.out_bytes, 1), dtype=torch.uint8, device=SP.device())
    torch.cuda.synchronize()
    return d_in, d_out


def bound_call(o, work, d_in, d_out):
    return lambda: work.call(o.ctx, o.res, d_in.data_ptr(), d_out.data_ptr())


def full_probe(o, work, **kw):
    """the probe on context o -> d_out as the stream saw it, through the work's view"""
    assert work.want != work.want_decoy, "the decoy would pass for the true input"
    d_in, d_out = buffers(work)
    got = SP.probe(o.ctx, o.s, bound_call(o, work, d_in, d_out), work.true_in, work.decoy_in, d_in, d_out, in_place=work.in_place,
                   warm=work.warm, **kw)
    return work.view(got)


# ---------------------------------------------------------------------------------------------- the tests
@pytest.mark.parametrize("name,variant", variants(QUEUED, [n for n in CASES if n not in MSM_CASES]))
def test_queued_entry_point_runs_on_the_callers_stream_and_does_not_wait(on_s, name, variant):
    work = CASES[name][1][variant]()
    assert full_probe(on_s, work) == work.want


@pytest.mark.parametrize("level", [0, 1, 2, 3])
@pytest.mark.parametrize("name,variant", variants(QUEUED, MSM_CASES))
def test_queued_msm_at_every_overlap_level(on_s, name, variant, level):
    """level 0: the caller's stream orders the result (the snapshot on s); 1 .. 3: the tails leave the stream and the header
    promises the result after h2agg_synchronize — the input side and the no-wait promise are the same at every level"""
    work = CASES[name][1][variant]()
    try:
        on_s.ctx.msm_set_tail_overlap(level)
        assert full_probe(on_s, work, after="stream" if level == 0 else "engine") == work.want
    finally:
        on_s.ctx.msm_set_tail_overlap(0)


@pytest.mark.parametrize("name,variant", variants(SYNCHRONOUS) + [(n, v) for n, vs in EXTRA_SYNCHRONOUS.items() for v in vs])
def test_synchronous_entry_point_reads_its_input_on_the_callers_stream(on_s, name, variant):
    work = (CASES[name][1] if name in CASES else EXTRA_SYNCHRONOUS[name])[variant]()
    assert work.want != work.want_decoy, "the decoy would pass for the true input"
    d_in, d_out = buffers(work)
    got = SP.probe_input_side(on_s.ctx, on_s.s, bound_call(on_s, work, d_in, d_out), work.true_in, work.decoy_in, d_in, warm=work.warm)
    assert got == work.want


def test_workspace_growth_inside_a_held_call(pkg):
    """a fresh context that has only seen k = 9: the transform at k = 12 replaces its twiddle table, which drains the device
    first (include/h2agg.h) — the call waits for the hold, and the result must still be the true input's"""
    k = 12
    a, d = fr_column(0xC001, 1 << k), fr_column(0xC002, 1 << k)
    o = OnStream(pkg)
    try:
        small = work_fft(False)
        assert full_probe(o, small) == small.want
        d_in = torch.zeros(32 << k, dtype=torch.uint8, device=SP.device())
        d_out = torch.zeros_like(d_in)
        call = lambda: o.ctx.fr_fft_device(d_in.data_ptr(), k, False, None, d_out.data_ptr())
        got = SP.probe(o.ctx, o.s, call, enc(a), enc(d), d_in, d_out, no_wait=False, warm=0)
        assert got == enc(Q.ntt(a, k))
    finally:
        o.close()


def test_stream_switch_to_the_own_stream_and_back(on_s):
    work = work_batch_invert()
    d_in, d_out = buffers(work)
    call = bound_call(on_s, work, d_in, d_out)
    try:
        on_s.ctx.set_stream(None)
        d_in.copy_(SP.to_device(work.true_in))
        d_out.fill_(SP.PATTERN)
        torch.cuda.synchronize()
        call()
        on_s.ctx.synchronize()
        assert SP.to_host(d_out) == work.want, "on the context's own stream"
    finally:
        on_s.ctx.set_stream(on_s.s.cuda_stream)
    assert full_probe(on_s, work) == work.want, "back on the caller's stream"


def test_set_stream_joins_a_deferred_tail(on_s):
    """overlap level 2, one 2^20-point MSM queued: its tail waits for the next call on the context.  h2agg_set_stream is that
    call: it joins the tails, so after it the device holds the result."""
    n = 1 << 20
    ks, kb = msm_scalars(0xD001, n)
    ss, sb = msm_scalars(0xD002, n)
    want = msm_point(ks, ss, n)
    ctx = on_s.ctx
    d_k, d_s = SP.to_device(kb), SP.to_device(sb)
    d_out = torch.full((96,), SP.PATTERN, dtype=torch.uint8, device=SP.device())
    torch.cuda.synchronize()
    table = ctx.bases_generate(d_k.data_ptr(), n)
    other = torch.cuda.Stream()
    try:
        ctx.msm_set_tail_overlap(2)
        ctx.g1_msm_device_async(table, d_s.data_ptr(), n, d_out.data_ptr())
        ctx.set_stream(other.cuda_stream)
        torch.cuda.synchronize()
        assert affine(SP.to_host(d_out)) == want
        ctx.synchronize()
    finally:
        ctx.msm_set_tail_overlap(0)
        ctx.set_stream(on_s.s.cuda_stream)
        ctx.bases_free(table)


def test_two_contexts_one_thread(pkg, on_s):
    """context A (on s_A, held) has a transform queued; the full probe on context B (on s_B) comes back with the right bytes
    while s_A is still held: nothing in a queued path waits for the device or for another context.  Then A's result.
    A's input is in place before the hold: a device-to-device copy queued behind A's hold would sit in front of B's copy in
    the runtime's copy path and could hold B up whatever the library does.  B's time is taken the moment s_B has drained,
    before anything is read back: a read-back runs on the default stream, whose hardware queue may be s_A's."""
    a_work, b_work = work_fft(False), work_columns_compress()
    s_a = on_s.s
    s_b = SP.stream_beside(lambda cand: (s_a, SP.torch_work(cand)))
    b = OnStream(pkg, s_b)
    try:
        a_in, a_out = buffers(a_work)
        a_call = bound_call(on_s, a_work, a_in, a_out)
        a_true, _bytes = SP.prepare(on_s.ctx, a_call, a_work.true_in, a_work.decoy_in, a_in, a_out)
        a_in.copy_(a_true)
        b_in, b_out = buffers(b_work)
        b_call = bound_call(b, b_work, b_in, b_out)
        b_true = SP.prepare(b.ctx, b_call, b_work.true_in, b_work.decoy_in, b_in, b_out)
        seen = {}
        t0 = time.perf_counter()
        with torch.cuda.stream(s_a):
            SP.hold(s_a, 4 * SP.HOLD_MS)
            a_call()
            a_snap = a_out.clone()

        def b_is_done():
            seen.update(a_busy=not s_a.query(), ms=1e3 * (time.perf_counter() - t0))
        got_b = SP.run(b.ctx, s_b, b_call, b_true, b_in, b_out, on_stream_done=b_is_done)
        assert seen["a_busy"], "context A's stream had drained before context B's: B waited for A"
        assert seen["ms"] < 3 * SP.HOLD_MS, "context B's stream took %.0f ms of context A's %d ms hold" % (seen["ms"], 4 * SP.HOLD_MS)
        assert got_b == b_work.want
        s_a.synchronize()
        assert SP.to_host(a_snap) == a_work.want
        on_s.ctx.synchronize()
    finally:
        b.close()


def test_the_probe_sees_a_context_that_is_not_on_the_held_stream(pkg):
    """the probe's own sharpness, and the only place where the unordered outcome is asserted: a context left on its OWN stream
    finishes while the held stream s has not even copied the true input, so its output is the decoy's"""
    work = work_fft(False)
    assert work.want != work.want_decoy
    ctx = pkg.H2Agg(0)
    try:
        d_in, d_out = buffers(work)
        call = lambda: work.call(ctx, None, d_in.data_ptr(), d_out.data_ptr())

        def finishes():
            call()
            ctx.synchronize()
        finishes()                                              # (the context's first call of this shape: its tables)
        s = SP.stream_beside(lambda cand: (cand, finishes))     # a stream whose queue the context's own stream does not share
        d_true, _bytes = SP.prepare(ctx, call, work.true_in, work.decoy_in, d_in, d_out)
        t0 = time.perf_counter()
        with torch.cuda.stream(s):
            SP.hold(s, SP.HOLD_MS)
            d_in.copy_(d_true, non_blocking=True)
        call()
        ctx.synchronize()
        took_ms = 1e3 * (time.perf_counter() - t0)
        assert not s.query(), "hold too short"
        assert took_ms < SP.HOLD_MS / 2, "hold too short: the context's own stream took %.1f ms, it queued behind the hold" % took_ms
        got = SP.to_host(d_out)
        s.synchronize()
        what = {work.want_decoy: "the decoy's", work.want: "the true input's", bytes([SP.PATTERN]) * len(got): "untouched"}
        assert got == work.want_decoy, "the output is %s" % what.get(got, "neither input's")
        assert SP.to_host(d_in) == work.true_in
    finally:
        ctx.close()
