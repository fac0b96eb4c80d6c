"""Test-side honest prover with every column RESIDENT: tests/honest_prover.py's driver over a backend that keeps the columns of
a proof in one Fr column store (h2agg_columns_*) instead of sending a slab across with every stage.

ResidentStages subclasses DeviceStages and answers the same interface (lists of integers in and out, because the driver
owns the transcript and the blinding).  Behind it a column crosses to the device ONCE: `where` remembers the store column of
every column the backend has written or produced, and a stage that is handed a known column gathers it with
h2agg_columns_move instead of writing it again.  Results are read back only because the driver wants integers; the next stage
finds them in the store.  The families with resident forms run through them (columns_fft, columns_commit, columns_sigmas,
columns_shplonk_begin is tests/test_gpu_columns.py's), every other family through its _device entry point over
h2agg_columns_ptr.  The proof must be the DeviceStages proof byte for byte (tests/test_gpu_columns.py)."""
from __future__ import annotations

from tests import honest_prover as HP
from tests import quotient_ref as Q
from tests.fr_bytes import dec, enc, fe
from tests.grand_product_ref import DELTA, R

CAPACITY = 512   # columns of the arena: a proof of the honest circuit places about 150


class ResidentStages(HP.DeviceStages):
    def __init__(self, pkg, eng, poly, verifier, setup):
        super().__init__(pkg, eng, poly, verifier, setup)
        self.k = setup.k
        self.arena = poly.ColumnStore(eng, CAPACITY, setup.k)
        self.top = 0
        self.where = {}          # a column's 32 * 2^k bytes -> the arena column that holds it
        self.writes = 0          # columns that crossed from the host
        self.moves = 0           # columns gathered on the device

    def close(self):
        if self.arena is not None:
            self.arena.close()
            self.arena = None
        super().close()

    # ---- the arena
    def _take(self, count):
        first = self.top
        assert first + count <= CAPACITY, "the arena is full"
        self.top += count
        return first

    def _slab(self, cols):
        """the columns (lists of integers) as one contiguous range of the arena -> its first column"""
        first = self._take(len(cols))
        for j, col in enumerate(cols):
            data = enc(col)
            at = self.where.get(data)
            if at is None:
                self.eng.columns_write(self.arena.handle, first + j, data)
                self.where[data] = first + j
                self.writes += 1
            else:
                self.eng.columns_move(self.arena.handle, at, self.arena.handle, first + j, 1, 0)
                self.moves += 1
        return first

    def _ptr(self, first):
        return self.eng.columns_ptr(self.arena.handle, first)

    def _result(self, first, count):
        """read a range the device has just written back as integers, and remember where it is"""
        out = self.arena.read(first, count)
        for j, data in enumerate(out):
            self.where.setdefault(data, first + j)
        return [dec(c) for c in out]

    def _blank(self, usable_rows, blinding):
        """a result column whose rows from usable_rows up are the blinding (or zero): the _device calls leave them alone"""
        n = 1 << self.k
        top = list(blinding[:n - usable_rows]) if blinding is not None else [0] * (n - usable_rows)
        first = self._take(1)
        self.eng.columns_write(self.arena.handle, first, enc([0] * usable_rows + top))
        return first

    # ---- keys
    def keygen(self, circuit):
        cs, k, u = circuit.cs, circuit.cs.k, circuit.usable
        m = len(cs.permutation_columns)
        h = self.arena.handle
        mapping = self.poly.permutation_mapping(m, k, u, circuit.copies)
        lag, coeff = self._take(m), self._take(m)
        self.eng.columns_sigmas(mapping, m, k, u, fe(DELTA), h, lag, h, coeff)
        sig_commit = self.eng.columns_commit(self.gl, h, lag, m)
        fixed = circuit.lag["fixed"]
        f_lag, f_coeff = self._slab(fixed), self._take(len(fixed))
        self.eng.columns_fft(h, f_lag, h, f_coeff, len(fixed), True)
        fixed_commit = self.eng.columns_commit(self.gl, h, f_lag, len(fixed))
        return HP.Key(self._result(lag, m), self._result(coeff, m), self._result(f_coeff, len(fixed)), self._points(fixed_commit),
                      self._points(sig_commit))

    # ---- commitments, domain
    def commit_coeff(self, cols, k):
        return self._points(self.eng.columns_commit(self.g, self.arena.handle, self._slab(cols), len(cols)))

    def commit_lagrange(self, cols, k):
        return self._points(self.eng.columns_commit(self.gl, self.arena.handle, self._slab(cols), len(cols)))

    def to_coeff(self, cols, k):
        src, dst = self._slab(cols), self._take(len(cols))
        self.eng.columns_fft(self.arena.handle, src, self.arena.handle, dst, len(cols), True)
        return self._result(dst, len(cols))

    # ---- lookup
    def compress(self, which, j, lag, theta):
        ptrs = [self._ptr(self._slab(lag[kind])) for kind in ("advice", "fixed", "instance")]
        out = self._take(1)
        self.eng.vk_expressions_eval_device(self.vk, which, j, self.k, *ptrs, None, fe(theta), self._ptr(out))
        return self._result(out, 1)[0]

    def permute(self, a, s, k, usable, blinding):
        d_a, d_s = self._ptr(self._slab([a])), self._ptr(self._slab([s]))
        ap = self._blank(usable, blinding[0] if blinding else None)
        sp = self._blank(usable, blinding[1] if blinding else None)
        self.eng.lookup_permute_device(d_a, d_s, k, usable, self._ptr(ap), self._ptr(sp))
        return self._result(ap, 1)[0], self._result(sp, 1)[0]

    # ---- grand products
    def permutation_products(self, values, sigmas, k, usable, beta, gamma, chunk_len, blinding):
        out, init = [], 1
        for s, lo in enumerate(range(0, len(values), chunk_len)):
            vs, ss = values[lo:lo + chunk_len], sigmas[lo:lo + chunk_len]
            d_v, d_s = self._ptr(self._slab(vs)), self._ptr(self._slab(ss))
            z = self._blank(usable + 1, blinding[s] if blinding else None)
            self.eng.permutation_product_device(d_v, d_s, len(vs), k, usable, fe(beta), fe(gamma), fe(DELTA), fe(pow(DELTA, lo, R)),
                                                fe(init), self._ptr(z))
            col = self._result(z, 1)[0]
            init = col[usable]
            out.append(col)
        return out

    def lookup_product(self, a, s, ap, sp, k, usable, beta, gamma, blinding):
        ptrs = [self._ptr(self._slab([c])) for c in (a, s, ap, sp)]
        z = self._blank(usable + 1, blinding)
        self.eng.lookup_product_device(*ptrs, k, usable, fe(beta), fe(gamma), self._ptr(z))
        return self._result(z, 1)[0]

    # ---- the quotient
    def quotient(self, polys, scalars):
        sc = scalars
        ptrs = [self._ptr(self._slab(polys[kind])) if polys[kind] else None for kind in Q.POLY_KINDS]
        pieces = self.vk.shape["degree"] - 1
        h = self._take(pieces)
        self.eng.quotient_device(self.vk, *ptrs, None, fe(sc["theta"]), fe(sc["beta"]), fe(sc["gamma"]), fe(sc["y"]), fe(sc["delta"]),
                                 self._ptr(h))
        return self._result(h, pieces)

    # ---- openings
    def evaluate(self, polys, k, queries, points):
        return dec(self.eng.fr_poly_eval_device(self._ptr(self._slab(polys)), len(polys), k, queries, enc(points)))

    def open(self, polys, k, queries, points, v):
        group_points, ws = self.eng.kzg_multiopen_device(self.g, self._ptr(self._slab(polys)), len(polys), k, queries, enc(points), fe(v))
        assert group_points == [pt for pt, _m in HP.group_queries(queries)]
        return self._points(ws)
