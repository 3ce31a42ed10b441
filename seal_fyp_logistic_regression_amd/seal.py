"""Host-side mirror of the Microsoft SEAL 3.4.5 API surface the reference drivers use, on top
of the hefx engine.  Same names, argument meaning and error behaviour as `seal::` so that tests read like the
reference's code (e.g. /root/reference/helper.h:237-262 becomes algorithms.linear_transform_plain).

Split of work: level/scale/parms_id bookkeeping, NAF decomposition of rotation steps and SEAL's validity checks
live here (host); all RNS arithmetic goes through a backend -- `GpuBackend` (the HIP engine; the only backend this
package ships) or, in tests only, an oracle-backed twin with the same methods.  Sampling (keys, noise) and the
complex FFT of CKKSEncoder run on the host in numpy; their NTTs run on the GPU.
"""
from __future__ import annotations

import math
import operator
import os
from typing import Dict, List, Optional, Sequence

import numpy as np

from . import capi
from .engine import Engine
from .poly import weight_residues


# ----------------------------------------------------------------------------------------------
# number theory helpers (host logic; CoeffModulus::Create, App. A.3)
# ----------------------------------------------------------------------------------------------
def _is_prime(n: int) -> bool:
    if n < 2:
        return False
    for p in (2, 3, 5, 7, 11, 13, 17, 19, 23, 29, 31, 37):
        if n % p == 0:
            return n == p
    d, r = n - 1, 0
    while d % 2 == 0:
        d //= 2
        r += 1
    for a in (2, 3, 5, 7, 11, 13, 17, 19, 23, 29, 31, 37):
        x = pow(a, d, n)
        if x in (1, n - 1):
            continue
        for _ in range(r - 1):
            x = x * x % n
            if x == n - 1:
                break
        else:
            return False
    return True


class CoeffModulus:
    @staticmethod
    def Create(poly_modulus_degree: int, bit_sizes: Sequence[int]) -> List[int]:
        """SEAL CoeffModulus::Create: per bit size walk down from 2^b - 2N + 1 in steps of 2N; primes of equal
        size are handed out smallest first (/root/reference/linear_transformation2.cpp:233)."""
        need: Dict[int, int] = {}
        for b in bit_sizes:
            if not 2 <= b <= 60:
                raise ValueError("bit_sizes is invalid")
            need[b] = need.get(b, 0) + 1
        table: Dict[int, List[int]] = {}
        for b, cnt in need.items():
            v, lower, found = (1 << b) - 2 * poly_modulus_degree + 1, 1 << (b - 1), []
            while len(found) < cnt and v > lower:
                if _is_prime(v):
                    found.append(v)
                v -= 2 * poly_modulus_degree
            if len(found) < cnt:
                raise ValueError("failed to find enough qualifying primes")
            table[b] = found
        return [table[b].pop() for b in bit_sizes]

    @staticmethod
    def BFVDefault(poly_modulus_degree: int) -> List[int]:
        """SEAL's hard-coded 128-bit-security defaults (util/globals.cpp) for the degrees the
        reference uses -- /root/reference/vector_ops.cpp:208 builds its CKKS context (BASELINE config 1) on this chain."""
        table = {
            4096: [0xffffee001, 0xffffc4001, 0x1ffffe0001],
            8192: [0x7fffffd8001, 0x7fffffc8001, 0xfffffffc001, 0xffffff6c001, 0xfffffebc001],
            16384: [0xfffffffd8001, 0xfffffffa0001, 0xfffffff00001, 0x1fffffff68001, 0x1fffffff50001,
                    0x1ffffffee8001, 0x1ffffffea0001, 0x1ffffffe88001, 0x1ffffffe48001],
        }
        if poly_modulus_degree not in table:
            raise ValueError("poly_modulus_degree is not supported by BFVDefault")
        return list(table[poly_modulus_degree])

    @staticmethod
    def MaxBitCount(poly_modulus_degree: int) -> int:
        return {1024: 27, 2048: 54, 4096: 109, 8192: 218, 16384: 438, 32768: 881}[poly_modulus_degree]


def galois_elt_from_step(step: int, N: int) -> int:
    """SEAL galois_elt_from_step (App. A.7)."""
    m = 2 * N
    if step == 0:
        return m - 1
    if abs(step) >= N // 2:
        raise ValueError("step count too large")
    pos = step if step > 0 else N // 2 + step
    return pow(3, pos, m)


def naf(value: int) -> List[int]:
    """SEAL util::naf: non-adjacent form, least significant term first, signed like `value`."""
    sign, value, res, i = value < 0, abs(value), [], 0
    while value:
        zi = 2 - (value & 3) if value & 1 else 0
        value = (value - zi) >> 1
        if zi:
            res.append((-zi if sign else zi) * (1 << i))
        i += 1
    return res


# ----------------------------------------------------------------------------------------------
# backend: the HIP engine
# ----------------------------------------------------------------------------------------------
class GpuBackend:
    """Adapter exposing the hefx C-ABI with handle-in / handle-out methods (handles are DeviceArray)."""

    name = "hip"

    def __init__(self, N: int, primes: Sequence[int], device: int = 0):
        self.engine = Engine(N, primes, device=device)
        self.N, self.primes, self.k = N, list(primes), len(primes)

    def from_host(self, a: np.ndarray):
        return self.engine.to_device(a)

    def to_host(self, h) -> np.ndarray:
        return h.download()

    def ntt_forward(self, h, npoly, nrows, mod_first=0):
        self.engine.ntt_forward(h, npoly, nrows, mod_first)
        return h

    def ntt_inverse(self, h, npoly, nrows, mod_first=0):
        self.engine.ntt_inverse(h, npoly, nrows, mod_first)
        return h

    def add(self, L, size, a, b):
        return self.engine.add(L, size, a, b)

    def sub(self, L, size, a, b):
        return self.engine.sub(L, size, a, b)

    def negate(self, L, size, a):
        return self.engine.negate(L, size, a)

    def add_plain(self, L, size, ct, pt):
        return self.engine.add_plain(L, size, ct, pt)

    def add_many(self, L, size, cts):
        return self.engine.add_many(L, size, cts)

    def multiply_plain(self, L, size, ct, pt):
        return self.engine.multiply_plain(L, size, ct, pt)

    def multiply_plain_sum(self, L, size, cts, pts, group=None):
        return self.engine.multiply_plain_sum(L, size, cts, pts, group)

    def scalar_combine(self, L, size, ins, in_rows, weights, consts=None):
        """outs[g] = sum_k weights[g][k] * ins[k] + consts[g] in one pass (hefx_scalar_combine; weights [G][m][L] and consts
        [G][L] are residues); the oracle-backed twin of the tests has no such method and Evaluator.scalar_combine composes
        the same words from mod_drop, multiply_plain, add_many and add_plain"""
        return self.engine.scalar_combine(L, size, ins, in_rows, weights, consts)

    def plain_combine(self, L, ins, pts):
        """outs[g] = sum_k pts[g][k] (.) ins[k] over the non-None plaintexts of row g in one pass (hefx_plain_combine); the
        oracle-backed twin of the tests has no such method and Evaluator.plain_combine takes multiply_plain_sum per output"""
        return self.engine.plain_combine(L, ins, pts)

    def product_combine(self, L, As, a_rows, Bs, b_rows, u, lins, lin_rows, w, c=None):
        """outs[i] = sum_p u[p] * (As[i][p] (x) Bs[i][p]) + sum_k w[k] * lins[i][k] + c at size 3 in one pass
        (hefx_product_combine; u [P][L], w [m][L] and c [L] are residues); the oracle-backed twin of the tests has no such
        method and Evaluator.product_combine composes the same words from mod_drop, multiply, multiply_plain, add_many, add
        and add_plain"""
        return self.engine.product_combine(L, As, a_rows, Bs, b_rows, u, lins, lin_rows, w, c)

    def multiply_batch(self, L, As, Bs):
        return self.engine.multiply_batch(L, As, Bs)

    def multiply_sum(self, L, As, Bs, group=None):
        return self.engine.multiply_sum(L, As, Bs, group)

    def add_batch(self, L, size, As, Bs):
        return self.engine.add_batch(L, size, As, Bs)

    def rescale_batch(self, L, size, cts):
        return self.engine.rescale_batch(L, size, cts)

    def relinearize_batch(self, L, ct3s, key):
        return self.engine.relinearize_batch(L, ct3s, key)

    def multiply(self, L, a, b):
        return self.engine.multiply(L, a, b)

    def square(self, L, a):
        return self.engine.square(L, a)

    def multiply_sizes(self, L, size_a, a, size_b, b):
        return self.engine.multiply_sizes(L, size_a, a, size_b, b)

    def multiply_sizes_batch(self, L, size_a, As, size_b, Bs):
        return self.engine.multiply_sizes_batch(L, size_a, As, size_b, Bs)

    def relinearize_sizes(self, L, size_in, size_out, ct, keys):
        """keys[p - 2]: the key of s^p (None where the set does not hold that power)"""
        return self.engine.relinearize_sizes(L, size_in, size_out, ct, keys)

    def addsub_unequal(self, L, size_a, a, size_b, b, sub):
        """a +/- b for ciphertexts of different sizes, on the device: the sum / difference of the leading min(size)
        polynomials goes into the result and the longer operand's tail is copied behind it -- negated when it is the
        subtrahend's.  The words of the operation on the shorter operand padded with zero polynomials."""
        e, N = self.engine, self.N
        lo, hi = min(size_a, size_b), max(size_a, size_b)
        out = e.empty(hi, L, N)
        (e.sub if sub else e.add)(L, lo, a, b, out=out.view(0, (lo, L, N)))
        big = a if size_a > size_b else b
        tail, dst = big.view(lo * L * N, (hi - lo, L, N)), out.view(lo * L * N, (hi - lo, L, N))
        if sub and big is b:
            e.negate(L, hi - lo, tail, out=dst)
        else:
            e.copy_raw(dst.ptr, tail.ptr, tail.nbytes)
        return out

    def apply_galois(self, L, ct, elt, key):
        return self.engine.apply_galois(L, ct, elt, key)

    def apply_galois_batch(self, L, cts, elts, keys):
        return self.engine.apply_galois_batch(L, cts, elts, keys)

    def rotate_multiply_plain_batch(self, L, cts, elts, keys, pts):
        return self.engine.rotate_multiply_plain_batch(L, cts, elts, keys, pts)

    def apply_galois_forest(self, L, parents, ext_ins, elts, keys, pts=None):
        """a forest of rotations in one engine call (hefx_apply_galois_forest); the oracle-backed twin of the tests has no
        such method and runs the same nodes depth by depth (algorithms._rotations_of_many)"""
        return self.engine.apply_galois_forest(L, parents, ext_ins, elts, keys, pts)

    def rotate_add_chain(self, L, cts, elts, keys, accs, steps):
        """`steps` x (t = apply_galois(t); a = a + t) per pair, in lockstep (helper.h:472-476 as one engine call)"""
        return self.engine.rotate_add_chain(L, cts, elts, keys, accs, steps)

    def relinearize(self, L, ct3, key):
        return self.engine.relinearize(L, ct3, key)

    def rescale(self, L, size, ct):
        return self.engine.rescale_to_next(L, size, ct)

    # floor (SEAL 3.4.x as SURVEY App. A.9 states it, default) or round-to-nearest (SEAL >= 3.5) division in
    # rescale_to_next: the one [M]-confidence semantic of the bit-exact path, switchable per context
    @property
    def rescale_rounded(self) -> bool:
        return self.engine.rescale_rounded

    @rescale_rounded.setter
    def rescale_rounded(self, v: bool):
        self.engine.set_rescale_rounded(bool(v))

    def mod_drop(self, L_in, L_out, npoly, x):
        return self.engine.mod_drop(L_in, L_out, npoly, x)

    def reduce_canonical(self, L, size, h, addends):
        return self.engine.reduce_canonical(L, size, h, addends)

    def linear_transform_plain(self, L, ct, diag_pts, key_elts, keys, hoisted=False):
        return self.engine.linear_transform_plain(L, ct, diag_pts, key_elts, keys, hoisted=hoisted)

    def linear_transform_plain_many(self, L, cts, diag_pts, key_elts, keys):
        return self.engine.linear_transform_plain_many(L, cts, diag_pts, key_elts, keys)

    def linear_transform_cipher(self, L, ct, diag_cts, key_elts, keys):
        return self.engine.linear_transform_cipher(L, ct, diag_cts, key_elts, keys)

    def rotate_hoisted_batch(self, L, ct, elts, keys, pts=None):
        return self.engine.rotate_hoisted_batch(L, ct, elts, keys, pts)

    def linear_transform_plain_hoisted2_sparse(self, L, ct, d, steps, diag_pts_keylevel, key_elts, keys):
        return self.engine.linear_transform_plain_hoisted2_sparse(L, ct, d, steps, diag_pts_keylevel, key_elts, keys)

    def linear_transform_plain_bsgs(self, L, ct, shifted_diag_pts, n1, key_elts, keys, hoisted=True):
        return self.engine.linear_transform_plain_bsgs(L, ct, shifted_diag_pts, n1, key_elts, keys, hoisted)

    def sample(self, kind, key32, stream_id, npoly, nrows, mod_first=0):
        return self.engine.sample(kind, key32, stream_id, npoly, nrows, mod_first)

    def keygen_kswitch(self, sk, new_sk, key32, stream_id):
        return self.engine.keygen_kswitch(sk, new_sk, key32, stream_id)

    def galois_permute(self, elt, a, rows):
        return self.engine.galois_permute(elt, a, rows)

    def encrypt(self, L, pk, plain, key32, stream_id):
        return self.engine.encrypt(L, pk, plain, key32, stream_id)

    def decrypt(self, L, size, ct, sk):
        return self.engine.decrypt(L, size, ct, sk)

    def mod_raise(self, L_in, L_out, x, count=1):
        return self.engine.mod_raise(L_in, L_out, x, count)

    def switch_key(self, L, ct, key):
        return self.engine.switch_key(L, ct, key)

    def collapse_key(self, L, key):
        return self.engine.collapse_key(L, key)

    def hybrid_keygen(self, alpha, sk, new_sk, key32, stream_id):
        return self.engine.hybrid_keygen(alpha, sk, new_sk, key32, stream_id)

    def hybrid_apply_galois_batch(self, alpha, L, cts, elts, keys):
        return self.engine.hybrid_apply_galois_batch(alpha, L, cts, elts, keys)

    def hybrid_relinearize_batch(self, alpha, L, ct3s, key):
        return self.engine.hybrid_relinearize_batch(alpha, L, ct3s, key)

    def hybrid_rotate_hoisted_batch(self, alpha, L, cts, elts, keys):
        return self.engine.hybrid_rotate_hoisted_batch(alpha, L, cts, elts, keys)

    def hybrid_plain_combine_hoisted(self, alpha, L, cts, elts, keys, pts):
        return self.engine.hybrid_plain_combine_hoisted(alpha, L, cts, elts, keys, pts)

    def hybrid_bsgs_hoisted(self, alpha, L, cts, elts, keys, pts, giant_elts, giant_keys, dest):
        return self.engine.hybrid_bsgs_hoisted(alpha, L, cts, elts, keys, pts, giant_elts, giant_keys, dest)

    def raise_switch(self, L_out, ct, ckey):
        """mod-raise from one prime and the collapsed key switch in one engine call (hefx_raise_switch); the oracle-backed
        twin of the tests has no such method and Evaluator.raise_switch states the same words through its apply_galois"""
        return self.engine.raise_switch(L_out, ct, ckey)

    def hybrid_collapse_key(self, alpha, L, key):
        return self.engine.hybrid_collapse_key(alpha, L, key)

    def hybrid_raise_switch(self, alpha, L_out, ct, ckey):
        """the same with a collapsed hybrid key (hefx_hybrid_raise_switch); the twin runs seal.hybrid_raise_switch_host"""
        return self.engine.hybrid_raise_switch(alpha, L_out, ct, ckey)

    def refresh(self, L_in, size, L_out, ct, sk, pk, key32, stream_id):
        """decrypt -> exact lift -> encrypt in one engine call (hefx_refresh); the oracle-backed twin of the tests has no
        such method and Decryptor.refresh composes the same words from its decrypt, transforms and encrypt"""
        return self.engine.refresh(L_in, size, L_out, ct, sk, pk, key32, stream_id)

    def refresh_batch(self, L_in, size, L_out, cts, sk, pk, key32, first_stream_id):
        return self.engine.refresh_batch(L_in, size, L_out, cts, sk, pk, key32, first_stream_id)

    def ckks_decode(self, L, pt, scale):
        return self.engine.ckks_decode(L, pt, scale)[0]

    def ckks_encode(self, L, values, scale):
        """[count][nvalues] slot values -> [count][L][N] NTT-form plaintexts, or None if N is outside the kernel's range"""
        if not 1024 <= self.N <= 32768:
            return None
        return self.engine.ckks_encode(L, values, scale)

    def ckks_encode_wide(self, L, values, scale):
        """ckks_encode for 2^62 <= max|v| * scale < 2^(bc-3) (hefx_ckks_encode_wide); None outside the kernel's range of N"""
        if not 1024 <= self.N <= 32768:
            return None
        return self.engine.ckks_encode_wide(L, values, scale)

    def ckks_encode_scalar(self, L, value, scale):
        """one scalar -> [L][N] plaintext with round(value * scale) mod q_j in every word (hefx_ckks_encode_scalar)"""
        return self.engine.ckks_encode_scalar(L, [value], scale).view(0, (L, self.N))


# ----------------------------------------------------------------------------------------------
# SEAL-shaped objects
# ----------------------------------------------------------------------------------------------
class EncryptionParameters:
    def __init__(self, scheme: str = "ckks"):
        if str(scheme).lower() != "ckks":
            raise ValueError("unsupported scheme (this engine implements the CKKS path only)")
        self._n = 0
        self._q: List[int] = []

    def set_poly_modulus_degree(self, n: int):
        self._n = int(n)

    def set_coeff_modulus(self, primes: Sequence[int]):
        self._q = [int(p) for p in primes]

    def poly_modulus_degree(self) -> int:
        return self._n

    def coeff_modulus(self) -> List[int]:
        return list(self._q)


class ContextData:
    def __init__(self, ctx: "SEALContext", parms_id: int):
        self._ctx, self._pid = ctx, parms_id

    def parms_id(self):
        return self._pid

    def chain_index(self) -> int:
        return self._pid - 1 if self._pid <= self._ctx.k - 1 or self._ctx.k == 1 else self._ctx.k - 1

    def coeff_modulus(self) -> List[int]:
        return self._ctx.primes[: self._pid]

    def total_coeff_modulus_bit_count(self) -> int:
        p = 1
        for q in self.coeff_modulus():
            p *= q
        return p.bit_length()

    def next_context_data(self):
        return ContextData(self._ctx, self._pid - 1) if self._pid > 1 else None


class SEALContext:
    """parms_id == number of RNS primes of the level: k for the key level, k-1 for the first data level ... 1."""

    def __init__(self, parms: EncryptionParameters, backend=None, device: int = 0):
        self.N = parms.poly_modulus_degree()
        self.primes = parms.coeff_modulus()
        self.k = len(self.primes)
        if self.N < 1024 or self.N & (self.N - 1):
            raise ValueError("poly_modulus_degree is not valid")
        self.backend = backend if backend is not None else GpuBackend(self.N, self.primes, device)

    @classmethod
    def Create(cls, parms, backend=None, device: int = 0):
        return cls(parms, backend, device)

    def key_parms_id(self) -> int:
        return self.k

    def first_parms_id(self) -> int:
        return self.k - 1 if self.k > 1 else 1

    def last_parms_id(self) -> int:
        return 1

    def key_context_data(self):
        return ContextData(self, self.k)

    def first_context_data(self):
        return ContextData(self, self.first_parms_id())

    def get_context_data(self, parms_id: int):
        return ContextData(self, parms_id)


class Plaintext:
    def __init__(self):
        self.data = None  # backend handle [L][N], NTT form
        self._parms_id = 0
        self._scale = 1.0
        self.is_zero = False  # known at encode time: lets multiply_plain raise "transparent" without a sync

    def parms_id(self):
        return self._parms_id

    @property
    def scale(self):
        return self._scale

    @scale.setter
    def scale(self, v):
        self._scale = float(v)


_PT_STATE = operator.attrgetter("_parms_id", "_scale", "is_zero")


class Ciphertext:
    def __init__(self):
        self.data = None  # backend handle [size][L][N], NTT form
        self._size = 0
        self._parms_id = 0
        self._scale = 1.0

    def size(self) -> int:
        return self._size

    def parms_id(self):
        return self._parms_id

    @property
    def scale(self):
        return self._scale

    @scale.setter
    def scale(self, v):
        self._scale = float(v)

    def _set(self, data, size, parms_id, scale):
        self.data, self._size, self._parms_id, self._scale = data, size, parms_id, float(scale)
        return self

    def copy(self) -> "Ciphertext":  # value semantics of seal::Ciphertext; payloads are never mutated in place
        return Ciphertext()._set(self.data, self._size, self._parms_id, self._scale)


class SecretKey:
    def __init__(self, host: np.ndarray, handle):
        self.host, self.data = host, handle  # [k][N] NTT form


class KSwitchKeys:
    """GaloisKeys / RelinKeys: index -> device key [k-1][2][k][N].  A Galois key sits under its Galois element, the
    relinearisation key of s^p under p - 2 (SEAL's RelinKeys::get_index; s^2, the only power a size-3 ciphertext needs,
    under 0)."""

    def __init__(self):
        self.keys: Dict[int, object] = {}

    def has_key(self, elt: int) -> bool:
        return elt in self.keys

    def key(self, elt: int):
        return self.keys[elt]

    # RelinKeys by power of the secret key
    @staticmethod
    def get_index(key_power: int) -> int:
        if key_power < 2:
            raise ValueError("key_power cannot be less than 2")
        return key_power - 2

    def has_power(self, key_power: int) -> bool:
        return key_power >= 2 and (key_power - 2) in self.keys

    def power_key(self, key_power: int):
        return self.keys[self.get_index(key_power)]


GaloisKeys = KSwitchKeys
RelinKeys = KSwitchKeys

HYBRID_ALPHA_MAX = 8  # HEFX_HYBRID_ALPHA_MAX (hefx_hybrid.h)


class HybridKeys(KSwitchKeys):
    """Keys of hybrid key switching (include/hefx_hybrid.h): alpha data primes per digit and the LAST alpha primes of the chain
    as special primes; index -> device key [dnum][2][k][N], dnum = ceil((k - alpha) / alpha), under the indices of KSwitchKeys
    (and under 1, the identity element, for Evaluator.switch_key).  Evaluator.rotate_vector, apply_galois, complex_conjugate,
    relinearize from size 3 and switch_key read them through hybrid_key(); ciphertexts must sit at a level <= k - alpha.  The
    fused composites (linear transforms, plain_combine / product_combine pipelines, the bootstrap) read their keys through
    key() / power_key(), which refuse here: their kernels know the one-special-prime layout only.  Many rotations of the same
    ciphertexts and their plaintext-weighted sums: Evaluator.rotate_hoisted / plain_combine_hoisted (include/hefx_hybrid_hoist.h)."""

    def __init__(self, alpha: int):
        super().__init__()
        self.alpha = int(alpha)

    def hybrid_key(self, index: int):
        return self.keys[index]

    def _refuse(self):
        raise TypeError(f"HybridKeys (alpha = {self.alpha}) with a fused composite or a size above 3 is not supported: hybrid key "
                        "switching serves rotate_vector, apply_galois, complex_conjugate, relinearize from size 3 and switch_key; "
                        "linear transforms, plain_combine / product_combine pipelines and the bootstrap need KSwitchKeys")

    def key(self, elt: int):
        self._refuse()

    def power_key(self, key_power: int):
        self._refuse()


def _hybrid_basis(primes: Sequence[int], alpha: int, L: int):
    """(q, S, rows, P) of include/hefx_hybrid.h: the chain, its special rows, the rows of a level-L switch, the special modulus"""
    q = [int(p) for p in primes]
    S = list(range(len(q) - alpha, len(q)))
    P = 1
    for t in S:
        P *= q[t]
    return q, S, list(range(L)) + S, P


def _row_ntt(be, q, m: int, v) -> np.ndarray:
    """one row of integers, reduced mod q[m], through the backend's forward transform -> Python integers"""
    return np.asarray(be.to_host(be.ntt_forward(be.from_host((v % q[m]).astype(np.uint64)[None, None]), 1, 1, m))).reshape(-1).astype(object)


def _row_intt(be, m: int, v) -> np.ndarray:
    """one canonical row through the backend's inverse transform -> Python integers"""
    return np.asarray(be.to_host(be.ntt_inverse(be.from_host(np.asarray(v, dtype=np.uint64)[None, None]), 1, 1, m))).reshape(-1).astype(object)


def _hybrid_digits_host(be, primes: Sequence[int], alpha: int, L: int, x: np.ndarray) -> List[Dict[int, np.ndarray]]:
    """Steps 1 to 3 of include/hefx_hybrid.h's statement: x [L][N] NTT form -> E[j][m], digit j extended to every row m of the
    switch (the digit's own rows are x's own)."""
    q, _, rows, _ = _hybrid_basis(primes, alpha, L)
    coef = [_row_intt(be, i, x[i]) for i in range(L)]
    E = []
    for j in range((L + alpha - 1) // alpha):
        G = list(range(j * alpha, min((j + 1) * alpha, L)))
        Dj = 1
        for i in G:
            Dj *= q[i]
        y = {i: coef[i] * pow(Dj // q[i], -1, q[i]) % q[i] for i in G}
        E.append({m: x[m].astype(object) if m in G else _row_ntt(be, q, m, sum(y[i] * ((Dj // q[i]) % q[m]) for i in G)) for m in rows})
    return E


def _hybrid_mod_down_host(be, primes: Sequence[int], alpha: int, L: int, B) -> np.ndarray:
    """Step 5: B[c, m] canonical over the rows of the switch -> round(B / P) [2][L][N]"""
    q, S, _, P = _hybrid_basis(primes, alpha, L)
    out = np.empty((2, L, len(B[0, 0])), dtype=np.uint64)
    for c in range(2):
        z = {t: (_row_intt(be, t, B[c, t].astype(np.uint64)) + (P // 2) % q[t]) % q[t] * pow(P // q[t], -1, q[t]) % q[t] for t in S}
        for j in range(L):
            v = sum(z[t] * ((P // q[t]) % q[j]) for t in S) % q[j]
            out[c, j] = ((B[c, j] - _row_ntt(be, q, j, v - (P // 2) % q[j])) * pow(P, -1, q[j]) % q[j]).astype(np.uint64)
    return out


def hybrid_switch_host(be, primes: Sequence[int], alpha: int, L: int, x: np.ndarray, key: np.ndarray) -> np.ndarray:
    """The switch of include/hefx_hybrid.h's statement, steps 1 to 5, in Python integers over the backend's own transforms:
    x [L][N] NTT form, key [dnum][2][k][N] -> ks [2][L][N].  What Evaluator runs with HybridKeys on a backend without the
    native entries (the oracle twin of the tests)."""
    q, _, rows, _ = _hybrid_basis(primes, alpha, L)
    N = np.asarray(x).shape[-1]
    key = np.asarray(key).reshape(-1, 2, len(q), N)
    E = _hybrid_digits_host(be, primes, alpha, L, np.asarray(x, dtype=np.uint64).reshape(L, N))
    return _hybrid_mod_down_host(be, primes, alpha, L, {(c, m): sum(E[j][m] * key[j, c, m].astype(object) for j in range(len(E))) % q[m]
                                                       for c in range(2) for m in rows})


def _hybrid_rows_add_host(primes: Sequence[int], ks: np.ndarray, add: np.ndarray) -> np.ndarray:
    """a copy of ks [2][L][N] with add[c, j] added mod q_j to its first len(add) polynomials, in Python integers"""
    out = ks.copy()
    for c in range(len(add)):
        for j in range(ks.shape[1]):
            out[c, j] = ((ks[c, j].astype(object) + add[c, j].astype(object)) % int(primes[j])).astype(np.uint64)
    return out


def hybrid_hoist_host(be, primes: Sequence[int], alpha: int, L: int, cts, elts, keys, pts=None) -> List[np.ndarray]:
    """The statement of include/hefx_hybrid_hoist.h in Python integers over the backend's own transforms.  cts: n arrays
    [2][L][N]; elts, keys: m elements and keys [dnum][2][k][N] (None with the element 1: the identity term).  pts None: the
    n * m hoisted rotations, out[i * m + k]; else pts[o][i * m + k] = a key-level plaintext [k][N] or None, and the G
    combined outputs, one mod-down each.  What Evaluator.rotate_hoisted / plain_combine_hoisted run on a backend without
    the native entries (the oracle twin of the tests)."""
    terms = _hybrid_terms_host(be, primes, alpha, L, cts, elts, keys)
    if pts is None:
        return [_hybrid_mod_down_host(be, primes, alpha, L, A) for A in terms]
    return [_hybrid_mod_down_host(be, primes, alpha, L, B) for B in _hybrid_sums_host(primes, alpha, L, terms, pts)]


def _hybrid_terms_host(be, primes: Sequence[int], alpha: int, L: int, cts, elts, keys) -> List[Dict]:
    """the terms A_t of include/hefx_hybrid_hoist.h, t = i * m + k, each {(c, m): row of Python integers} over the rows of R"""
    from . import galois_tables
    q, _, rows, P = _hybrid_basis(primes, alpha, L)
    k, N = len(q), np.asarray(cts[0]).shape[-1]
    terms = []                                             # A_t: {(c, m): row}
    for ct in cts:
        ct = np.asarray(ct, dtype=np.uint64).reshape(2, L, N)
        E = _hybrid_digits_host(be, primes, alpha, L, ct[1])  # the digits of c1, not permuted
        for elt, key in zip(elts, keys):
            A = {}
            if key is None:
                if elt != 1:
                    raise ValueError("hybrid hoisting: a missing key denotes the identity term: its element must be 1")
                for c in range(2):
                    for m in rows:
                        A[c, m] = ct[c, m].astype(object) * (P % q[m]) % q[m] if m < L else np.zeros(N, dtype=object)
            else:
                key = np.asarray(key).reshape(-1, 2, k, N)
                g = galois_tables.gather_table(N, elt)
                for c in range(2):
                    for m in rows:
                        A[c, m] = sum(E[j][m][g] * key[j, c, m].astype(object) for j in range(len(E))) % q[m]
                for m in range(L):
                    A[0, m] = (A[0, m] + (P % q[m]) * ct[0, m][g].astype(object)) % q[m]
            terms.append(A)
    return terms


def _hybrid_sums_host(primes: Sequence[int], alpha: int, L: int, terms, pts) -> List[Dict]:
    """the combine's sums B_o of include/hefx_hybrid_hoist.h over the rows of R, before their mod-down"""
    q, _, rows, _ = _hybrid_basis(primes, alpha, L)
    k, N = len(q), len(terms[0][0, 0])
    sums = []
    for row in pts:
        if len(row) != len(terms) or all(p is None for p in row):
            raise ValueError("hybrid hoisting: one plaintext (or None) per term, and a term per output")
        live = [(np.asarray(p, dtype=np.uint64).reshape(k, N), A) for p, A in zip(row, terms) if p is not None]
        sums.append({(c, m): sum(p[m].astype(object) * A[c, m] for p, A in live) % q[m] for c in range(2) for m in rows})
    return sums


def hybrid_bsgs_host(be, primes: Sequence[int], alpha: int, L: int, cts, elts, keys, pts, giant_elts, giant_keys, dest) -> List[np.ndarray]:
    """The statement of include/hefx_hybrid_bsgs.h in Python integers over the backend's own transforms.  The arguments of
    hybrid_hoist_host up to pts describe the G inner sums B_o; inner sum o is rotated in the extended basis by giant_elts[o]
    with giant_keys[o] ([dnum][2][k][N]; None with the element 1: W_o = B_o) and added into output dest[o]; the
    max(dest) + 1 outputs take one mod-down each.  What Evaluator.bsgs_hoisted runs on a backend without the native entry
    (the oracle twin of the tests)."""
    from . import galois_tables
    q, _, rows, _ = _hybrid_basis(primes, alpha, L)
    k = len(q)
    sums = _hybrid_sums_host(primes, alpha, L, _hybrid_terms_host(be, primes, alpha, L, cts, elts, keys), pts)
    if not (len(giant_elts) == len(giant_keys) == len(dest) == len(sums)):
        raise ValueError("hybrid bsgs: one giant element, giant key and dest per inner sum")
    O = max(int(d) for d in dest) + 1
    if min(int(d) for d in dest) < 0 or set(int(d) for d in dest) != set(range(O)):
        raise ValueError("hybrid bsgs: dest out of range, or an output has no inner sum")
    N = len(sums[0][0, 0])
    W = [{(c, m): np.zeros(N, dtype=object) for c in range(2) for m in rows} for _ in range(O)]
    for B, elt, key, d in zip(sums, giant_elts, giant_keys, dest):
        if (key is None) != (elt == 1):
            raise ValueError("hybrid bsgs: a missing giant key means no giant rotation: it goes with the element 1, and only with it")
        if key is None:
            Wo = B
        else:
            key = np.asarray(key).reshape(-1, 2, k, N)
            g = galois_tables.gather_table(N, elt)
            # MD of the ONE polynomial B_o[1] (the mod-down is per polynomial: B_o[1] stands in for both), then its digits
            d1 = _hybrid_mod_down_host(be, primes, alpha, L, {(c, m): B[1, m] for c in range(2) for m in rows})[1]
            F = _hybrid_digits_host(be, primes, alpha, L, d1)
            Wo = {(c, m): sum(F[j][m][g] * key[j, c, m].astype(object) for j in range(len(F))) % q[m] for c in range(2) for m in rows}
            for m in rows:
                Wo[0, m] = (Wo[0, m] + B[0, m][g]) % q[m]
        for c in range(2):
            for m in rows:
                W[int(d)][c, m] = (W[int(d)][c, m] + Wo[c, m]) % q[m]
    return [_hybrid_mod_down_host(be, primes, alpha, L, Wq) for Wq in W]


class EncapsKeys:
    """The two switching keys of sparse-secret encapsulation (KeyGenerator.encapsulation_keys): `low` takes a ciphertext at
    the last prime from the main secret s to the auxiliary sparse secret s' (zero outside digit 0, rows {0, k-1}: it lives
    at modulus q_0 P), `high` takes one at any level from s' back to s.  s' itself is not kept.  The collapsed form of
    `high` that Evaluator.raise_switch reads is cached here per level."""

    def __init__(self, low, high, hamming_weight: int):
        self.low, self.high, self.hamming_weight = low, high, int(hamming_weight)
        self._collapsed: Dict[int, object] = {}


def collapse_key_host(key: np.ndarray, primes: Sequence[int], L: int) -> np.ndarray:
    """The collapsed key of level L on the host: key [k-1][2][k][N] -> [2][k][N], row m the sum of the first L digits' rows m
    mod q_m (hefx_collapse_key keeps the rows 0 .. L-1 and k-1 of it).  Exact in uint64: canonical words of primes below
    2^61, reduced after every addition."""
    k = len(primes)
    key = np.asarray(key, dtype=np.uint64).reshape(k - 1, 2, k, -1)
    q = np.asarray([int(p) for p in primes], dtype=np.uint64)[None, :, None]
    out = key[0].copy()
    for j in range(1, L):
        out += key[j]
        out -= np.where(out >= q, q, np.uint64(0))
    return out


class HybridEncapsKeys:
    """The two switching keys of sparse-secret encapsulation on hybrid keys (KeyGenerator.hybrid_encapsulation_keys).  `low`
    is an ORDINARY key [k-1][2][k][N], word for word encapsulation_keys(...).low: it takes a ciphertext at the last prime from
    the main secret s to the auxiliary sparse secret s' and lives at modulus q_0 q_(k-1) (zero outside digit 0, rows {0, k-1}).
    `high` is a HybridKeys(alpha) holding, under the element 1, the hybrid key [dnum][2][k][N] of s' -> s: an encryption under
    the MAIN secret at the full modulus q_0 ... q_(k-1), alpha special primes.  s' itself is not kept.  The collapsed forms of
    `high` that Evaluator.raise_switch reads (include/ext/hefx_hybrid_encaps.h) are cached here per level."""

    def __init__(self, low, high: "HybridKeys", hamming_weight: int):
        self.low, self.high, self.hamming_weight = low, high, int(hamming_weight)
        self._collapsed: Dict[int, object] = {}


def hybrid_collapse_key_host(key: np.ndarray, primes: Sequence[int], alpha: int, L: int) -> np.ndarray:
    """hefx_hybrid_collapse_key on the host: key [dnum][2][k][N] -> [2][L + alpha][N], row r the sum of the first
    ceil(L / alpha) digits' rows m(r) mod q_m(r) (r < L: data prime r, else special prime k - alpha + r - L).  Exact in
    uint64: canonical words of primes below 2^61, reduced after every addition."""
    q, _, rows, _ = _hybrid_basis(primes, alpha, L)
    key = np.asarray(key, dtype=np.uint64).reshape(-1, 2, len(q), np.asarray(key).shape[-1])
    qr = np.asarray([q[m] for m in rows], dtype=np.uint64)[None, :, None]
    out = key[0][:, rows].copy()
    for j in range(1, (L + alpha - 1) // alpha):
        out += key[j][:, rows]
        out -= np.where(out >= qr, qr, np.uint64(0))
    return out


def hybrid_raise_switch_host(be, primes: Sequence[int], alpha: int, L: int, ct: np.ndarray, ckey: np.ndarray) -> np.ndarray:
    """The statement of include/ext/hefx_hybrid_encaps.h in Python integers over the backend's own transforms: ct [2][1][N] at
    q_0, ckey [2][L + alpha][N] (hybrid_collapse_key_host) -> [2][L][N].  x, y: the centred lifts of c1, c0 (lift_coefficients);
    acc[c][r] = NTT(x mod q_m(r)) ckey[c][r] over the L + alpha rows; the hybrid mod-down (_hybrid_mod_down_host); y added to
    polynomial 0.  What Evaluator.raise_switch runs with HybridEncapsKeys on a backend without the native entry (the oracle
    twin of the tests)."""
    q, _, rows, _ = _hybrid_basis(primes, alpha, L)
    ct = np.asarray(ct, dtype=np.uint64).reshape(2, 1, -1)
    N = ct.shape[2]
    ckey = np.asarray(ckey, dtype=np.uint64).reshape(2, L + alpha, N)
    coef = np.asarray(be.to_host(be.ntt_inverse(be.from_host(ct.copy()), 2, 1, 0))).reshape(2, N)
    lifted = [lift_coefficients(coef[p][None], [q[0]] + [q[m] for m in rows[1:]], 1, len(rows)) for p in range(2)]  # rows[1:] of y, x
    x = {0: ct[1, 0].astype(object)}
    y = np.empty((1, L, N), dtype=np.uint64)
    y[0, 0] = ct[0, 0]
    for r, m in enumerate(rows[1:]):
        x[m] = _row_ntt(be, q, m, lifted[1][r].astype(object))
        if m < L:
            y[0, m] = _row_ntt(be, q, m, lifted[0][r].astype(object)).astype(np.uint64)
    B = {(c, m): x[m] * ckey[c, r].astype(object) % q[m] for c in range(2) for r, m in enumerate(rows)}
    return _hybrid_rows_add_host(primes, _hybrid_mod_down_host(be, primes, alpha, L, B), y)


CT_SIZE_MAX = 16  # HEFX_CT_SIZE_MAX (hefx.h): the most polynomials a ciphertext may have in this engine


def _c_round(x):
    """C's round() -- halves away from zero, what SEAL's encoder calls -- for every double: numpy array in, float64 array
    of integers out; a Python float in, a Python int out.  (np.rint and Python's round() send halves to the even
    neighbour; floor(x + 0.5) is wrong at 0.49999999999999994 and above 2^52.)  x - trunc(x) is exact in float64."""
    if isinstance(x, float):
        t = math.trunc(x)
        return t + (0 if abs(x - t) < 0.5 else (1 if x > 0 else -1))
    t = np.trunc(x)
    return t + np.where(np.abs(x - t) >= 0.5, np.sign(x), 0.0)


def _key32(seed) -> bytes:
    """32-byte ChaCha20 key of the backend sampler: fresh OS randomness when seed is None (production), else a
    deterministic expansion of the integer seed (tests: randomness is an input of the parity chain)."""
    import hashlib
    if seed is None:
        return os.urandom(32)
    return hashlib.sha256(b"hefx-seed:" + str(int(seed)).encode()).digest()


def sparse_ternary_secret(key32: bytes, N: int, hamming_weight: int) -> np.ndarray:
    """The coefficients (int64, in {-1, 0, 1}) of a secret with exactly hamming_weight nonzero entries, a function of key32
    alone: positions by a partial Fisher-Yates shuffle, then one sign bit each, both from the SHA-256 counter stream of
    key32 (64-bit words, a word outside the largest multiple of the range is drawn again: no modulo bias).  Host only."""
    import hashlib
    h = int(hamming_weight)
    if not 1 <= h <= N:
        raise ValueError("hamming_weight must lie in 1 .. poly_modulus_degree")
    state = {"ctr": 0, "buf": []}

    def word() -> int:
        if not state["buf"]:
            d = hashlib.sha256(b"hefx-sparse-secret:" + key32 + state["ctr"].to_bytes(8, "little")).digest()
            state["ctr"] += 1
            state["buf"] = [int.from_bytes(d[i:i + 8], "little") for i in range(0, 32, 8)]
        return state["buf"].pop()

    def below(r: int) -> int:
        limit = (1 << 64) - (1 << 64) % r
        while True:
            w = word()
            if w < limit:
                return w % r

    idx = list(range(N))
    for i in range(h):
        j = i + below(N - i)
        idx[i], idx[j] = idx[j], idx[i]
    out = np.zeros(N, dtype=np.int64)
    for i in range(h):
        out[idx[i]] = 1 if word() & 1 else -1
    return out


class KeyGenerator:
    """Randomness from the backend's counter-mode sampler (hefx_sample_*: ChaCha20 keystream, SEAL 3.4.5's
    distributions; SEAL seeds from random_device, so keys are inputs to parity, never outputs); all modular
    arithmetic on the backend (App. A.11).  The default seed=None draws the sampler key from the OS (os.urandom);
    an integer seed is for tests and tools only -- it makes the secret key publicly derivable.
    hamming_weight=h: a sparse secret with exactly h entries of +-1 (sparse_ternary_secret, drawn on the host from the same
    key32) in place of the uniform ternary one -- what bootstrapping needs: the integer part I of a mod-raised plaintext
    m + q_0 I has about (h + 1) / 12 of variance per coefficient, and EvalMod's range K must cover it.  The sampler streams of
    every other key are what they are without it.  None: the uniform ternary secret, word for word as before."""

    def __init__(self, context: SEALContext, seed: Optional[int] = None, hamming_weight: Optional[int] = None):
        self.ctx = context
        self._key32, self._stream = _key32(seed), 0
        be, k = context.backend, context.k
        if hamming_weight is None:
            h = be.sample("ternary", self._key32, 2 * self._next_stream(), 1, k)
        else:
            self._next_stream()  # (the uniform secret's stream stays unused: the other keys keep their stream ids)
            coef = sparse_ternary_secret(self._key32, context.N, hamming_weight)
            h = be.from_host(np.stack([(coef % int(q)).astype(np.uint64) for q in context.primes[:k]])[None])
        be.ntt_forward(h, 1, k, 0)
        self._sk = SecretKey(be.to_host(h).reshape(k, context.N), h)

    def _next_stream(self) -> int:
        self._stream += 1
        return self._stream

    def secret_key(self) -> SecretKey:
        return self._sk

    def _encrypt_zero(self, npoly: int, rows: int, sid: int, sk: Optional[SecretKey] = None, key32: Optional[bytes] = None):
        """npoly fresh symmetric encryptions of zero over the first `rows` primes: returns host (c0, c1);
        a uniform from sampler stream 2*sid, e noise from 2*sid+1 (what hefx_keygen_kswitch draws).  sk, key32: another
        secret and sampler key than the generator's own (encapsulation_keys)"""
        be, sk = self.ctx.backend, sk if sk is not None else self._sk
        key32 = key32 if key32 is not None else self._key32
        a = be.sample("uniform", key32, 2 * sid, npoly, rows)
        e = be.sample("noise", key32, 2 * sid + 1, npoly, rows)
        be.ntt_forward(e, npoly, rows, 0)
        sk_rows = be.from_host(sk.host[:rows])
        as_ = be.multiply_plain(rows, npoly, a, sk_rows)
        c0 = be.negate(rows, npoly, be.add(rows, npoly, as_, e))
        return (be.to_host(c0).reshape(npoly, rows, self.ctx.N),
                be.to_host(a).reshape(npoly, rows, self.ctx.N))

    def public_key(self):
        # generated once, like SEAL's KeyGenerator (public_key() returns the same key on every call)
        if getattr(self, "_pk", None) is None:
            c0, c1 = self._encrypt_zero(1, self.ctx.k, self._next_stream())
            self._pk = np.stack([c0[0], c1[0]])  # [2][k][N]
        return self._pk

    def _kswitch_key(self, new_sk_host, new_sk_dev=None, sk: Optional[SecretKey] = None, key32: Optional[bytes] = None,
                     sid: Optional[int] = None):
        """key-switching key for new_sk under sk.  On the HIP engine: one call (hefx_keygen_kswitch -- sampling, NTT and
        assembly on the device); otherwise the same arithmetic composed from backend ops (the oracle twin in tests:
        same sampler streams, same bits).  sk, key32, sid (all three: encapsulation_keys): a key under another secret, from a
        sampler key and stream id of its own -- the generator's stream counter stays where it is."""
        ctx, be = self.ctx, self.ctx.backend
        k, N, q = ctx.k, ctx.N, ctx.primes
        if sid is None:
            sid = self._next_stream()
        sk = sk if sk is not None else self._sk
        key32 = key32 if key32 is not None else self._key32
        native = getattr(be, "keygen_kswitch", None)
        if native is not None:
            if new_sk_dev is None:
                new_sk_dev = be.from_host(new_sk_host)
            return native(sk.data, new_sk_dev, key32, sid)
        if new_sk_host is None:
            new_sk_host = be.to_host(new_sk_dev).reshape(k, N)
        c0, c1 = self._encrypt_zero(k - 1, k, sid, sk, key32)
        P = q[k - 1]
        # c0[i][row i] += (P mod q_i) * new_sk[row i]
        factor = np.empty((k, N), dtype=np.uint64)
        for j in range(k):
            factor[j, :] = P % q[j]
        t = be.to_host(be.multiply_plain(k, 1, be.from_host(new_sk_host[None]), be.from_host(factor)))[0]
        for i in range(k - 1):
            s = c0[i, i] + t[i]
            c0[i, i] = np.where(s >= q[i], s - q[i], s)
        key = np.stack([c0, c1], axis=1)  # [k-1][2][k][N]
        return be.from_host(key)

    def relin_keys(self, count: int = 1) -> KSwitchKeys:
        """keys of s^2 .. s^(count + 1) (KeyGenerator::relin_keys(count)): what relinearising a ciphertext of up to
        count + 2 polynomials needs.  The powers are formed on the device; the sampler stream ids are taken in increasing
        power, so relin_keys(1) is the key relin_keys() always gave."""
        if count < 1 or count > CT_SIZE_MAX - 2:
            raise ValueError("invalid count")
        be, sk = self.ctx.backend, self._sk
        rk = KSwitchKeys()
        power = be.from_host(sk.host[None])
        for p in range(2, count + 2):
            power = be.multiply_plain(self.ctx.k, 1, power, sk.data)
            rk.keys[p - 2] = self._kswitch_key(None, power)
        return rk

    def _hybrid_key(self, alpha: int, new_sk_host, new_sk_dev=None, sk: Optional[SecretKey] = None, key32: Optional[bytes] = None,
                    sid: Optional[int] = None):
        """hybrid switching key [dnum][2][k][N] for new_sk under the generator's secret: hefx_hybrid_keygen on the HIP engine,
        otherwise the same words composed from backend operations as _kswitch_key does (a dnum-polynomial draw from the
        sub-streams 2 sid, 2 sid + 1; F_j = P mod q_m on the data rows of digit j).  sk, key32, sid: as in _kswitch_key
        (hybrid_encapsulation_keys) -- with a sid given the generator's stream counter stays where it is."""
        ctx, be = self.ctx, self.ctx.backend
        k, N, q = ctx.k, ctx.N, [int(p) for p in ctx.primes]
        if sid is None:
            sid = self._next_stream()
        sk = sk if sk is not None else self._sk
        key32 = key32 if key32 is not None else self._key32
        native = getattr(be, "hybrid_keygen", None)
        if native is not None:
            return native(alpha, sk.data, new_sk_dev if new_sk_dev is not None else be.from_host(new_sk_host), key32, sid)
        if new_sk_host is None:
            new_sk_host = be.to_host(new_sk_dev).reshape(k, N)
        D = k - alpha
        dnum = (D + alpha - 1) // alpha
        c0, c1 = self._encrypt_zero(dnum, k, sid, sk, key32)
        P = 1
        for t in range(D, k):
            P *= q[t]
        factor = np.empty((k, N), dtype=np.uint64)
        for m in range(k):
            factor[m, :] = P % q[m]
        t = be.to_host(be.multiply_plain(k, 1, be.from_host(np.asarray(new_sk_host)[None]), be.from_host(factor)))[0]
        for j in range(dnum):
            for m in range(j * alpha, min((j + 1) * alpha, D)):
                s = c0[j, m] + t[m]
                c0[j, m] = np.where(s >= q[m], s - q[m], s)
        return be.from_host(np.stack([c0, c1], axis=1))

    def _check_alpha(self, alpha: int) -> int:
        alpha = int(alpha)
        if alpha < 1 or alpha >= self.ctx.k or alpha > HYBRID_ALPHA_MAX:
            raise ValueError(f"hybrid keys: alpha must lie in 1 .. min(k - 1, {HYBRID_ALPHA_MAX}), k = {self.ctx.k}")
        return alpha

    def hybrid_relin_keys(self, alpha: int) -> "HybridKeys":
        """the hybrid relinearisation key of s^2 (index 0): the last alpha primes of the chain are special primes"""
        alpha = self._check_alpha(alpha)
        be, sk = self.ctx.backend, self._sk
        rk = HybridKeys(alpha)
        rk.keys[0] = self._hybrid_key(alpha, None, be.multiply_plain(self.ctx.k, 1, be.from_host(sk.host[None]), sk.data))
        return rk

    def hybrid_galois_keys(self, alpha: int, steps: Optional[Sequence[int]] = None, conjugate: bool = False) -> "HybridKeys":
        """galois_keys(steps, conjugate) as hybrid keys: the same elements in the same order, one sampler stream each"""
        from . import galois_tables
        alpha = self._check_alpha(alpha)
        N = self.ctx.N
        elts = self.default_galois_elts() if steps is None else [galois_elt_from_step(s, N) for s in steps]
        if conjugate and 2 * N - 1 not in elts:
            elts = elts + [2 * N - 1]
        gk = HybridKeys(alpha)
        permute = getattr(self.ctx.backend, "galois_permute", None)
        for g in elts:
            if permute is not None:
                gk.keys[g] = self._hybrid_key(alpha, None, permute(g, self._sk.data, self.ctx.k))
            else:
                gk.keys[g] = self._hybrid_key(alpha, self._sk.host[:, galois_tables.gather_table(N, g)])
        return gk

    def hybrid_switching_key(self, alpha: int, from_secret: "SecretKey") -> "HybridKeys":
        """the hybrid key that takes a ciphertext under from_secret to this generator's secret, under the identity element 1
        (Evaluator.switch_key)"""
        alpha = self._check_alpha(alpha)
        sw = HybridKeys(alpha)
        sw.keys[1] = self._hybrid_key(alpha, from_secret.host, from_secret.data)
        return sw

    def encapsulation_keys(self, hamming_weight: int = 32, seed: Optional[int] = None) -> EncapsKeys:
        """The keys of sparse-secret encapsulation (Bossuat, Troncoso-Pastoriza, Hubaux, ACNS 2022) for bootstrapping under
        THIS generator's secret s, which may be dense: an auxiliary secret s' of exactly hamming_weight entries of +-1
        (sparse_ternary_secret) is drawn from a sampler key of its own -- seed=None: from the OS; an integer: tests only --
        and two switching keys are made, both from that sampler key (streams 1 and 2; the generator's other keys keep their
        stream ids).  low: s -> s' (hefx_keygen_kswitch(sk = s', new_sk = s)), of which a key switch at the last prime reads
        digit 0, rows {0, k-1} only; every other word is zeroed before the key leaves the generator, so nothing under s' at
        the full modulus is published.  high: s' -> s, under the main secret.  s' is not kept on the result."""
        key32 = _key32(seed)
        aux, low = self._encaps_low(hamming_weight, key32)
        high = self._kswitch_key(aux.host, aux.data, key32=key32, sid=2)
        return EncapsKeys(low, high, hamming_weight)

    def _encaps_low(self, hamming_weight: int, key32: bytes):
        """(s', low) of encapsulation_keys and hybrid_encapsulation_keys: the auxiliary secret of key32 and the ordinary key
        s -> s' from stream 1 of key32, zeroed outside digit 0, rows {0, k-1}"""
        ctx, be = self.ctx, self.ctx.backend
        k, N = ctx.k, ctx.N
        if k < 2:
            raise ValueError("encapsulation_keys: key switching needs a special prime")
        coef = sparse_ternary_secret(key32, N, hamming_weight)
        h = be.from_host(np.stack([(coef % int(q)).astype(np.uint64) for q in ctx.primes[:k]])[None])
        be.ntt_forward(h, 1, k, 0)
        aux = SecretKey(np.array(be.to_host(h), dtype=np.uint64).reshape(k, N), h)
        low = np.array(be.to_host(self._kswitch_key(self._sk.host, self._sk.data, sk=aux, key32=key32, sid=1)),
                       dtype=np.uint64).reshape(k - 1, 2, k, N)
        keep = low[0][:, [0, k - 1]].copy()
        low[:] = 0
        low[0][:, [0, k - 1]] = keep
        return aux, be.from_host(low)

    def hybrid_encapsulation_keys(self, alpha: int, hamming_weight: int = 32, seed: Optional[int] = None) -> HybridEncapsKeys:
        """encapsulation_keys for a program on HYBRID keys (algorithms.bootstrap_hybrid(..., encaps=)): the same auxiliary
        secret s' (sparse_ternary_secret of the sampler key of `seed`, exactly hamming_weight entries of +-1) and the same two
        sampler streams of that key, 1 and 2; the generator's stream counter does not move and s' is not kept.
        low: word for word encapsulation_keys(hamming_weight, seed).low -- an ORDINARY key, zero outside digit 0, rows
        {0, k-1}: it lives at modulus q_0 q_(k-1).  The switch at the last prime is Evaluator.switch_key at L = 1
        (hefx_switch_key), which needs nothing hybrid, and the sparse secret stays at that small modulus instead of q_0 times
        alpha special primes.
        high: HybridKeys(alpha) with the hybrid key of s' -> s under the element 1 (hefx_hybrid_keygen, or the composed form on
        a backend without it), an encryption under the main secret at the full modulus q_0 ... q_(k-1), the last alpha primes
        special; at alpha = 1 its words are encapsulation_keys(...).high.
        The collapsed forms Evaluator.raise_switch reads are cached on the result per level.  No security claim is made for
        either modulus or for the weight of s'."""
        alpha = self._check_alpha(alpha)
        key32 = _key32(seed)
        aux, low = self._encaps_low(hamming_weight, key32)
        high = HybridKeys(alpha)
        high.keys[1] = self._hybrid_key(alpha, aux.host, aux.data, key32=key32, sid=2)
        return HybridEncapsKeys(low, high, hamming_weight)

    def default_galois_elts(self) -> List[int]:
        N = self.ctx.N
        logn = N.bit_length() - 1
        elts = [2 * N - 1]
        for i in range(logn - 1):
            elts += [pow(3, 1 << i, 2 * N), pow(3, N // 2 - (1 << i), 2 * N)]
        return sorted(set(elts))

    def galois_keys(self, steps: Optional[Sequence[int]] = None, conjugate: bool = False) -> KSwitchKeys:
        """keygen.galois_keys(): default = 3^(+-2^i) and 2N-1 (power-of-two steps only, App. A.7).  conjugate=True adds the
        key of the Galois element 2N - 1 (Evaluator.complex_conjugate) behind the keys of `steps`, whose sampler streams
        stay what they are without it; the default set already holds it."""
        from . import galois_tables
        N = self.ctx.N
        elts = self.default_galois_elts() if steps is None else [galois_elt_from_step(s, N) for s in steps]
        if conjugate and 2 * N - 1 not in elts:
            elts = elts + [2 * N - 1]
        gk = KSwitchKeys()
        permute = getattr(self.ctx.backend, "galois_permute", None)
        for g in elts:
            if permute is not None:  # s(X^g) on the device
                gk.keys[g] = self._kswitch_key(None, permute(g, self._sk.data, self.ctx.k))
            else:
                tab = galois_tables.gather_table(N, g)
                gk.keys[g] = self._kswitch_key(self._sk.host[:, tab])
        return gk


class Encryptor:
    """(pk0*u + e0 + m, pk1*u + e1) over the plaintext's level in ONE engine call (hefx_encrypt: sampling, NTT and
    the dyadic arithmetic all on the GPU).  The default seed=None draws the sampler key from the OS;
    an integer seed (tests only) replays the same (u, e0, e1) for the i-th ciphertext of every such instance."""

    def __init__(self, context: SEALContext, public_key: np.ndarray, seed: Optional[int] = None):
        self.ctx, self.pk = context, public_key
        self._pk_dev = context.backend.from_host(np.ascontiguousarray(public_key))  # [2][k][N]
        self._key32, self._stream = _key32(seed), 0

    def encrypt(self, plain: Plaintext, destination: Optional[Ciphertext] = None) -> Ciphertext:
        L = plain.parms_id()
        self._stream += 1
        c = self.ctx.backend.encrypt(L, self._pk_dev, plain.data, self._key32, self._stream)
        out = destination if destination is not None else Ciphertext()
        return out._set(c, 2, L, plain.scale)


class Decryptor:
    def __init__(self, context: SEALContext, secret_key: SecretKey):
        self.ctx, self.sk = context, secret_key

    def decrypt(self, encrypted: Ciphertext, destination: Optional[Plaintext] = None) -> Plaintext:
        """c0 + c1 s (+ c2 s^2): handles size-3 ciphertexts (/root/reference/matrix_multiplication.cpp:419);
        one engine call (hefx_decrypt)."""
        L = encrypted.parms_id()
        out = destination if destination is not None else Plaintext()
        out.data = self.ctx.backend.decrypt(L, encrypted.size(), encrypted.data, self.sk.data)
        out._parms_id, out._scale = L, encrypted.scale
        return out

    # ---- refresh: decrypt, lift to a higher level, encrypt.  What the reference's training loop does after every step
    # (logistic_regression_ckks.cpp:362-381), without its decode / encode pair: at one scale that pair is the identity on
    # the integer polynomial, so the plaintext's centred coefficients are written mod the target level's primes -- exact.
    def _refresh_target(self, encrypted: Ciphertext, parms_id: Optional[int]) -> int:
        L_out = parms_id if parms_id is not None else self.ctx.first_parms_id()
        if encrypted.size() < 2:
            raise ValueError("encrypted is not valid for encryption parameters")
        if L_out < encrypted.parms_id() or L_out > self.ctx.first_parms_id():
            raise ValueError("refresh: the target level must lie between the ciphertext's and the first level")
        return L_out

    def _refresh_composed(self, encrypted: Ciphertext, encryptor: "Encryptor", L_out: int, stream_id: int):
        """the words of the engine's refresh from a backend without one: decrypt, inverse transform, lift_coefficients,
        forward transform of the new rows, encrypt"""
        be, N, L_in = self.ctx.backend, self.ctx.N, encrypted.parms_id()
        pt = be.decrypt(L_in, encrypted.size(), encrypted.data, self.sk.data)
        if L_in < L_out:
            old = np.array(be.to_host(pt), dtype=np.uint64).reshape(L_in, N)
            coef = np.asarray(be.to_host(be.ntt_inverse(be.from_host(old), 1, L_in, 0))).reshape(L_in, N)
            new = be.ntt_forward(be.from_host(lift_coefficients(coef, self.ctx.primes, L_in, L_out)), 1, L_out - L_in, L_in)
            pt = be.from_host(np.concatenate([old, np.asarray(be.to_host(new)).reshape(L_out - L_in, N)]))
        return be.encrypt(L_out, encryptor._pk_dev, pt, encryptor._key32, stream_id)

    def refresh(self, encrypted: Ciphertext, encryptor: "Encryptor", parms_id: Optional[int] = None) -> Ciphertext:
        """A fresh size-2 encryption, at level parms_id (default: the first level), of what `encrypted` decrypts to; the
        scale is unchanged.  The encryptor's stream counter advances as encrypt() advances it.  One engine call
        (hefx_refresh) when the backend has it."""
        L_out = self._refresh_target(encrypted, parms_id)
        encryptor._stream += 1
        native = getattr(self.ctx.backend, "refresh", None) if self.ctx.N <= 16384 else None  # (the entry's range of N)
        if native is not None:
            data = native(encrypted.parms_id(), encrypted.size(), L_out, encrypted.data, self.sk.data, encryptor._pk_dev,
                          encryptor._key32, encryptor._stream)
        else:
            data = self._refresh_composed(encrypted, encryptor, L_out, encryptor._stream)
        return Ciphertext()._set(data, 2, L_out, encrypted.scale)

    def refresh_many(self, encrypteds: Sequence[Ciphertext], encryptor: "Encryptor",
                     parms_id: Optional[int] = None) -> List[Ciphertext]:
        """[refresh(c) for c in encrypteds], the same words and stream ids, as one engine call (hefx_refresh_batch) when the
        ciphertexts share level and size and the backend has it"""
        cts = list(encrypteds)
        native = getattr(self.ctx.backend, "refresh_batch", None) if self.ctx.N <= 16384 else None
        if not cts or native is None or any(c.parms_id() != cts[0].parms_id() or c.size() != cts[0].size() for c in cts):
            return [self.refresh(c, encryptor, parms_id) for c in cts]
        L_out = self._refresh_target(cts[0], parms_id)
        first = encryptor._stream + 1
        encryptor._stream += len(cts)
        outs = native(cts[0].parms_id(), cts[0].size(), L_out, [c.data for c in cts], self.sk.data, encryptor._pk_dev,
                      encryptor._key32, first)
        return [Ciphertext()._set(o, 2, L_out, c.scale) for o, c in zip(outs, cts)]


def lift_coefficients(rows: np.ndarray, primes: Sequence[int], L_in: int, L_out: int) -> np.ndarray:
    """The centred lift on the host, in Python integers: rows [L_in][N] (coefficient form, canonical) -> the new rows
    L_in .. L_out-1, [L_out - L_in][N].  Every coefficient x in [0, Q_in), Q_in = q_0 ... q_(L_in-1), stands for x when
    x <= Q_in // 2 and for x - Q_in otherwise (Q_in is odd: no tie) -- the rule of CKKSEncoder.decode -- and is written
    mod the new primes.  Composed by Garner's mixed-radix digits; the engine's kernel (hefx_mod_raise) does the same work
    in 64-bit residues."""
    q = [int(p) for p in primes]
    rows = np.asarray(rows).reshape(L_in, -1)
    digits = []
    for j in range(L_in):  # d_j = ((r_j - d_0) q_0^-1 - d_1) q_1^-1 ... mod q_j
        t = rows[j].astype(object)
        for i in range(j):
            t = (t - digits[i]) * pow(q[i], -1, q[j]) % q[j]
        digits.append(t)
    x, Q = digits[-1], q[L_in - 1]
    for i in range(L_in - 2, -1, -1):  # x = d_0 + q_0 (d_1 + q_1 (d_2 + ...))
        x, Q = x * q[i] + digits[i], Q * q[i]
    x = np.where((x > Q // 2).astype(bool), x - Q, x)
    out = np.empty((L_out - L_in, rows.shape[1]), dtype=np.uint64)
    for j in range(L_in, L_out):
        out[j - L_in] = (x % q[j]).astype(np.uint64)
    return out


class CKKSEncoder:
    """Canonical embedding with slot i <-> root zeta^(3^i) (App. A.12).  encode runs on the GPU
    (hefx_ckks_encode: FFT + rounding + RNS + NTT in two launches; hefx_ckks_encode_wide from max|v| * scale = 2^62 up to
    2^(bc-3), bc the bit count of the level's modulus; hefx_ckks_encode_scalar for scalars) when the backend offers it;
    anything beyond uses the host FFT + the backend NTT.  device_encode=False forces the host path (bit-identical across
    backends -- what the evaluator parity tests use)."""

    def __init__(self, context: SEALContext, device_encode: bool = True):
        self.ctx = context
        self.device_encode = bool(device_encode)
        N = context.N
        pos = np.empty(N // 2, dtype=np.int64)
        p = 1
        for i in range(N // 2):
            pos[i] = p
            p = p * 3 % (2 * N)
        self._r1 = (pos - 1) >> 1
        self._r2 = (2 * N - pos - 1) >> 1
        self._zeta = np.exp(1j * np.pi * np.arange(N) / N)

    def slot_count(self) -> int:
        return self.ctx.N // 2

    def _to_rns(self, coeffs: np.ndarray, L: int) -> np.ndarray:
        q = self.ctx.primes
        out = np.empty((L, self.ctx.N), dtype=np.uint64)
        if np.abs(coeffs).max(initial=0.0) < 2.0 ** 62:
            ci = coeffs.astype(np.int64)
            for j in range(L):
                out[j] = np.mod(ci, q[j]).astype(np.uint64)
        else:  # wide coefficients (scale > 2^62): exact big-int path
            ci = [int(c) for c in coeffs]
            for j in range(L):
                out[j] = np.array([c % q[j] for c in ci], dtype=np.uint64)
        return out

    def encode(self, values, scale: float, destination: Optional[Plaintext] = None,
               parms_id: Optional[int] = None) -> Plaintext:
        ctx, be, N = self.ctx, self.ctx.backend, self.ctx.N
        L = parms_id if parms_id is not None else ctx.first_parms_id()
        out = destination if destination is not None else Plaintext()
        if np.isscalar(values):  # encode(double, scale, pt): every NTT slot = round(v*scale) mod q
            x = float(values) * float(scale)
            c = _c_round(x) if math.isfinite(x) else None
            bc = ContextData(ctx, L).total_coeff_modulus_bit_count()
            dev = getattr(be, "ckks_encode_scalar", None) if self.device_encode else None
            if dev is not None and c is not None and scale > 0 and abs(x) < 2.0 ** max(62, min(bc - 3, 1000)):
                out.data, out.is_zero = dev(L, float(values), float(scale)), c == 0
            else:
                c = _c_round(x)  # (a non-finite product raises here, as it always did)
                rows = np.empty((L, N), dtype=np.uint64)
                for j in range(L):
                    rows[j, :] = c % ctx.primes[j]
                out.data, out.is_zero = be.from_host(rows), c == 0
        else:
            v = np.asarray(values)
            if v.size > N // 2:
                raise ValueError("values has invalid size")
            dev = self._encode_device(v.reshape(1, -1), scale, L) if v.size else None
            if dev is not None:
                out.data, out.is_zero = dev[0].view(0, (L, N)), dev[1][0]
                out._parms_id, out._scale = L, float(scale)
                return out
            v = v.astype(np.complex128)
            A = np.zeros(N, dtype=np.complex128)
            A[self._r1[: v.size]] = v
            A[self._r2[: v.size]] = np.conj(v)
            a = np.fft.fft(A) / N
            coeffs = _c_round(np.real(a * np.conj(self._zeta)) * scale)
            rows = self._to_rns(coeffs, L)
            out.is_zero = not coeffs.any()
            out.data = be.ntt_forward(be.from_host(rows), 1, L, 0)
        out._parms_id, out._scale = L, float(scale)
        if math.log2(scale) >= ContextData(ctx, L).total_coeff_modulus_bit_count():
            raise ValueError("scale out of bounds")
        return out

    def _encode_device(self, v2d: np.ndarray, scale: float, L: int):
        """GPU encode when the backend has it: hefx_ckks_encode when every coefficient provably fits 62 bits and
        zero-ness is decidable from norms, hefx_ckks_encode_wide for 2^62 <= max|v| * scale < 2^(bc-3) (never zero);
        returns (slab [count][L][N], is_zero[count]) or None -> host path."""
        be, N = self.ctx.backend, self.ctx.N
        enc = getattr(be, "ckks_encode", None) if self.device_encode else None
        bc = ContextData(self.ctx, L).total_coeff_modulus_bit_count()
        if enc is None or not (scale > 0) or math.log2(scale) >= bc:
            return None
        mag = np.abs(v2d)
        if not np.all(np.isfinite(mag)):
            return None
        top = float(mag.max(initial=0.0)) * scale
        if top >= 2.0 ** 62:  # |p_k| <= max|v|: wide coefficients
            wide = getattr(be, "ckks_encode_wide", None)
            if wide is None or not top < 2.0 ** min(bc - 3, 1000):
                return None  # beyond the wide entry's bound: the exact big-int host path
            # Parseval as below: some row may still be (near) zero; only rows with a provably nonzero coefficient go
            lo = np.sqrt(2.0 * (mag.astype(np.float64) ** 2).sum(axis=1)) / N * scale
            if not np.all(lo > 0.501):
                return None
            slab = wide(L, v2d, scale)
            return None if slab is None else (slab, [False] * v2d.shape[0])
        # Parseval: sum p_k^2 = (2/N) sum |v_i|^2, so max|p_k| >= sqrt(2 sum|v|^2)/N; and max|p_k| <= max|v|
        hi = mag.max(axis=1) * scale
        lo = np.sqrt(2.0 * (mag.astype(np.float64) ** 2).sum(axis=1)) / N * scale
        zero, nonzero = hi < 0.499, lo > 0.501
        if not np.all(zero | nonzero):
            return None
        slab = enc(L, v2d, scale)
        if slab is None:
            return None
        return slab, [bool(z) for z in zero]

    def encode_many(self, vectors, scale: float, parms_id: Optional[int] = None) -> List[Plaintext]:
        """Encodes equally long vectors in one launch (the d diagonals of Linear_Transform_Plain,
        matrix_mult_benchmark.cpp:291-323; the one-hot masks of logistic_regression_ckks.cpp:222-225)."""
        ctx, N = self.ctx, self.ctx.N
        L = parms_id if parms_id is not None else ctx.first_parms_id()
        vs = [np.asarray(v) for v in vectors]
        if vs and all(v.ndim == 1 and v.size == vs[0].size and 0 < v.size <= N // 2 for v in vs):
            dev = self._encode_device(np.stack(vs), scale, L)
            if dev is not None:
                outs = []
                for i in range(len(vs)):
                    pt = Plaintext()
                    pt.data, pt.is_zero = dev[0].view(i * L * N, (L, N)), dev[1][i]
                    pt._parms_id, pt._scale = L, float(scale)
                    outs.append(pt)
                return outs
        return [self.encode(v, scale, None, L) for v in vs]

    def decode(self, plain: Plaintext) -> np.ndarray:
        ctx, be, N, L = self.ctx, self.ctx.backend, self.ctx.N, plain.parms_id()
        dev = getattr(be, "ckks_decode", None) if self.device_encode else None
        if dev is not None and L <= 16:  # inverse NTT, CRT, centring and the slot-root FFT on the GPU
            return dev(L, plain.data, plain.scale)
        h = be.from_host(be.to_host(plain.data))
        rows = be.to_host(be.ntt_inverse(h, 1, L, 0))
        q = ctx.primes[:L]
        Q = 1
        for p in q:
            Q *= p
        acc = np.zeros(N, dtype=object)
        for j in range(L):  # CRT compose
            Qj = Q // q[j]
            acc = (acc + rows[j].astype(object) * (Qj * pow(Qj, -1, q[j]))) % Q
        centered = np.array([float(c - Q) if c > Q // 2 else float(c) for c in acc]) / plain.scale
        A = np.fft.ifft(centered * self._zeta) * N
        return A[self._r1]


class Evaluator:
    """seal::Evaluator for CKKS.  Out-of-place forms return the destination; *_inplace forms rebind the
    ciphertext's payload (payload buffers are immutable once produced, so copies are O(1))."""

    def __init__(self, context: SEALContext):
        self.ctx, self.be = context, context.backend
        self._bitcount: Dict[int, int] = {}

    # ---- checks shared with SEAL
    @staticmethod
    def _close(a: float, b: float) -> bool:
        return abs(a - b) <= max(abs(a), abs(b)) * 2.0 ** -40 or a == b

    def _check_same(self, a, b):
        if a.parms_id() != b.parms_id():
            raise ValueError("encrypted1 and encrypted2 parameter mismatch")

    def _check_scale(self, new_scale: float, parms_id: int):
        bits = self._bitcount.get(parms_id)
        if bits is None:
            bits = self._bitcount[parms_id] = ContextData(self.ctx, parms_id).total_coeff_modulus_bit_count()
        if new_scale <= 0 or int(math.log2(new_scale)) >= bits:
            raise ValueError("scale out of bounds")

    def _plain_product_scale(self, L: int, ct_scale: float, pts: Sequence["Plaintext"], pt_level: int) -> float:
        """The checks multiply_plain + add_many make over ct (.) pts[i] for a ciphertext at level L and scale ct_scale, and
        the common product scale.  pt_level is the level the plaintexts must sit at: L, or the key level for the
        double-hoisted transforms.  Per plaintext the order is multiply_plain's -- level, scale bound, closeness to the
        first product, transparency -- and the FIRST offending plaintext raises, like the op-by-op sequence; every
        composite states its plaintext checks through this function, so an input with two faults reports the one
        multiply_plain would.  One set comparison when everything is in order (a 1000-diagonal transform is otherwise
        host-bound in this loop); the element-by-element walk only runs to raise."""
        if set(map(_PT_STATE, pts)) == {(pt_level, pts[0]._scale, False)}:  # (one C-level pass: 25 us for 512 plaintexts)
            scale = ct_scale * pts[0]._scale
            self._check_scale(scale, L)
            return scale
        scale = None
        for p in pts:
            if p.parms_id() != pt_level:
                raise ValueError("encrypted_ntt and plain_ntt parameter mismatch" if pt_level == L else
                                 "double hoisting needs key-level plaintexts (encode with parms_id = key level)")
            s = ct_scale * p.scale
            self._check_scale(s, L)
            if scale is not None and not self._close(scale, s):
                raise ValueError("scale mismatch")
            scale = s if scale is None else scale
            if p.is_zero:
                raise RuntimeError("result ciphertext is transparent")
        return scale

    # ---- add / sub / negate
    def _addsub(self, a: Ciphertext, b: Ciphertext, sub: bool) -> Ciphertext:
        self._check_same(a, b)
        if not self._close(a.scale, b.scale):
            raise ValueError("scale mismatch")
        L = a.parms_id()
        native = getattr(self.be, "addsub_unequal", None)
        if a.size() != b.size() and native is not None:  # result size = max; the extra polys are copied (negated for b in sub)
            size = max(a.size(), b.size())
            return Ciphertext()._set(native(L, a.size(), a.data, b.size(), b.data, sub), size, L, a.scale)
        if a.size() != b.size():  # the same through the host, for a backend without that route
            big, small = (a, b) if a.size() > b.size() else (b, a)
            hb = self.be.to_host(big.data)
            pad = np.zeros_like(hb)
            pad[: small.size()] = self.be.to_host(small.data)
            small = Ciphertext()._set(self.be.from_host(pad), big.size(), L, small.scale)
            a, b = (big, small) if a.size() > b.size() else (small, big)
        f = self.be.sub if sub else self.be.add
        return Ciphertext()._set(f(L, a.size(), a.data, b.data), a.size(), L, a.scale)

    def add(self, a, b, destination=None):
        r = self._addsub(a, b, False)
        return r if destination is None else destination._set(r.data, r.size(), r.parms_id(), r.scale)

    def add_inplace(self, a, b):
        return self.add(a, b, a)

    def sub(self, a, b, destination=None):
        r = self._addsub(a, b, True)
        return r if destination is None else destination._set(r.data, r.size(), r.parms_id(), r.scale)

    def sub_inplace(self, a, b):
        return self.sub(a, b, a)

    def add_many(self, cts: Sequence[Ciphertext], destination=None):
        """SEAL: destination = cts[0]; add_inplace the rest.  Same bits from one n-way reduction kernel."""
        if not cts:
            raise ValueError("encrypteds cannot be empty")
        for c in cts[1:]:
            self._check_same(cts[0], c)
            if not self._close(cts[0].scale, c.scale):
                raise ValueError("scale mismatch")
            if c.size() != cts[0].size():
                raise ValueError("add_many: mixed sizes are not supported by the fused reduction")
        L, size = cts[0].parms_id(), cts[0].size()
        data = self.be.add_many(L, size, [c.data for c in cts])
        out = destination if destination is not None else Ciphertext()
        return out._set(data, size, L, cts[0].scale)

    def negate(self, a, destination=None):
        out = destination if destination is not None else Ciphertext()
        return out._set(self.be.negate(a.parms_id(), a.size(), a.data), a.size(), a.parms_id(), a.scale)

    def negate_inplace(self, a):
        return self.negate(a, a)

    def add_plain(self, a: Ciphertext, p: Plaintext, destination=None):
        if a.parms_id() != p.parms_id():
            raise ValueError("encrypted and plain parameter mismatch")
        if not self._close(a.scale, p.scale):
            raise ValueError("scale mismatch")
        out = destination if destination is not None else Ciphertext()
        return out._set(self.be.add_plain(a.parms_id(), a.size(), a.data, p.data), a.size(), a.parms_id(), a.scale)

    def add_plain_inplace(self, a, p):
        return self.add_plain(a, p, a)

    # ---- multiply
    def multiply_plain(self, a: Ciphertext, p: Plaintext, destination=None):
        if a.parms_id() != p.parms_id():
            raise ValueError("encrypted_ntt and plain_ntt parameter mismatch")
        new_scale = a.scale * p.scale
        self._check_scale(new_scale, a.parms_id())
        data = self.be.multiply_plain(a.parms_id(), a.size(), a.data, p.data)
        if p.is_zero:
            raise RuntimeError("result ciphertext is transparent")  # SEAL: std::logic_error
        out = destination if destination is not None else Ciphertext()
        return out._set(data, a.size(), a.parms_id(), new_scale)

    def multiply_plain_inplace(self, a, p):
        return self.multiply_plain(a, p, a)

    # ---- the same operation over many independent ciphertexts (the rows of a data set): one engine launch per
    # list where the backend offers it, otherwise the per-item calls -- identical checks and bits either way
    def _uniform(self, cts):
        if not cts:  # an empty list is trivially uniform; the callers below return before touching cts[0]
            return True
        L, size, scale = cts[0].parms_id(), cts[0].size(), cts[0].scale
        return all(c._parms_id == L and c._size == size and c._scale == scale for c in cts)

    def multiply_many(self, As: Sequence[Ciphertext], Bs: Sequence[Ciphertext]) -> List[Ciphertext]:
        if not As:  # a rank that owns no unit of a sharded product (parallel.py)
            return []
        f = getattr(self.be, "multiply_batch", None)
        if f is None or not (self._uniform(As) and self._uniform(Bs)) or any(a.data is b.data for a, b in zip(As, Bs)):
            return [self.multiply(a, b) for a, b in zip(As, Bs)]
        a, b = As[0], Bs[0]
        self._check_same(a, b)
        if a.size() != 2 or b.size() != 2:
            raise ValueError("multiply: only size-2 operands are supported (all reference call sites)")
        s = a.scale * b.scale
        self._check_scale(s, a.parms_id())
        outs = f(a.parms_id(), [x.data for x in As], [x.data for x in Bs])
        return [Ciphertext()._set(o, 3, a.parms_id(), s) for o in outs]

    def relinearize_many_inplace(self, cts: Sequence[Ciphertext], relin_keys: KSwitchKeys):
        f = getattr(self.be, "relinearize_batch", None)
        if not cts:
            return cts
        if isinstance(relin_keys, HybridKeys):
            native = getattr(self.be, "hybrid_relinearize_batch", None)
            if native is None or len(cts) < 2 or not self._uniform(cts) or cts[0].size() != 3:
                for c in cts:
                    self.relinearize_inplace(c, relin_keys)
                return cts
            # a uniform batch from size 3: ONE call, whose words are those of the single calls (items are independent)
            if not relin_keys.has_key(0):
                raise ValueError("not enough relinearization keys")
            L = self._hybrid_level(cts[0], relin_keys)
            for c, o in zip(cts, native(relin_keys.alpha, L, [c.data for c in cts], relin_keys.hybrid_key(0))):
                c._set(o, 2, L, c.scale)
            return cts
        if f is None or not self._uniform(cts) or cts[0].size() != 3:
            for c in cts:
                self.relinearize_inplace(c, relin_keys)
            return cts
        L = cts[0].parms_id()
        for c, o in zip(cts, f(L, [c.data for c in cts], relin_keys.key(0))):
            c._set(o, 2, L, c.scale)
        return cts

    def rescale_to_next_many_inplace(self, cts: Sequence[Ciphertext]):
        f = getattr(self.be, "rescale_batch", None)
        if not cts:
            return cts
        if f is None or not self._uniform(cts) or cts[0].parms_id() < 2:
            for c in cts:
                self.rescale_to_next_inplace(c)
            return cts
        L, size = cts[0].parms_id(), cts[0].size()
        new_scale = cts[0].scale / float(self.ctx.primes[L - 1])
        for c, o in zip(cts, f(L, size, [c.data for c in cts])):
            c._set(o, size, L - 1, new_scale)
        return cts

    def add_pairs(self, As: Sequence[Ciphertext], Bs: Sequence[Ciphertext]) -> List[Ciphertext]:
        f = getattr(self.be, "add_batch", None)
        if not As:
            return []
        if f is None or not (self._uniform(As) and self._uniform(Bs)) or As[0].size() != Bs[0].size():
            return [self.add(a, b) for a, b in zip(As, Bs)]
        a, b = As[0], Bs[0]
        self._check_same(a, b)
        if not self._close(a.scale, b.scale):
            raise ValueError("scale mismatch")
        outs = f(a.parms_id(), a.size(), [x.data for x in As], [x.data for x in Bs])
        return [Ciphertext()._set(o, a.size(), a.parms_id(), a.scale) for o in outs]

    def multiply_plain_sum(self, cts: Sequence[Ciphertext], pts: Sequence[Plaintext], group: Optional[int] = None):
        """add_many(multiply_plain(cts[i], pts[i])) per group of `group` consecutive terms (None: one group), in one
        pass over the operands (hefx_multiply_plain_sum).  Checks and exceptions of the op-by-op sequence
        (helper.h:271,275), same bits.  Returns the list of group sums."""
        if not cts or len(cts) != len(pts):
            raise ValueError("multiply_plain_sum: need as many plaintexts as ciphertexts")
        L, size = cts[0].parms_id(), cts[0].size()
        if any(a._parms_id != L or a._size != size for a in cts):
            raise ValueError("encrypted parameter mismatch")
        if len({a._scale for a in cts}) == 1:
            scale = self._plain_product_scale(L, cts[0].scale, pts, L)
        else:  # ciphertexts at several scales: term by term, each product held to the first
            scale = self._plain_product_scale(L, cts[0].scale, pts[:1], L)
            for a, p in zip(cts[1:], pts[1:]):
                if not self._close(scale, self._plain_product_scale(L, a.scale, [p], L)):
                    raise ValueError("scale mismatch")
        outs = self.be.multiply_plain_sum(L, size, [a.data for a in cts], [p.data for p in pts], group)
        return [Ciphertext()._set(o, size, L, scale) for o in outs]

    def scalar_combine(self, cts: Sequence[Ciphertext], weights, wscales: Sequence[float], consts=None,
                       scale: Optional[float] = None, parms_id: Optional[int] = None) -> List[Ciphertext]:
        """G scalar combinations of the same ciphertexts: out[g] = sum_k weights[g][k] * cts[k] + consts[g], at level
        parms_id (default: the lowest level among cts; higher inputs are read through their row prefix) and scale S.
        weights: [G][m] floats (or [m] for one output); weight (g, k) is the scalar plaintext encode(weights[g][k],
        wscales[k]), so cts[k].scale * wscales[k] must be S for every k -- S is `scale` when given, else
        cts[0].scale * wscales[0]; consts: [G] floats encoded at S, or None.
        The words and the checks of the op-by-op sequence -- mod_switch_to, encode, multiply_plain per term, add_many,
        add_plain -- from ONE pass over the inputs where the backend has hefx_scalar_combine, else from that sequence."""
        cts = list(cts)
        W = np.atleast_2d(np.asarray(weights, dtype=np.float64))
        m, G = len(cts), W.shape[0]
        if m < 1 or W.shape[1] != m or len(wscales) != m:
            raise ValueError("scalar_combine: need one weight per output and ciphertext, one weight scale per ciphertext")
        cvals = None if consts is None else np.atleast_1d(np.asarray(consts, dtype=np.float64))
        if cvals is not None and cvals.shape != (G,):
            raise ValueError("scalar_combine: need one constant per output")
        L = int(parms_id) if parms_id is not None else min(c.parms_id() for c in cts)
        size = cts[0].size()
        S = float(scale) if scale is not None else cts[0].scale * float(wscales[0])
        wres = self._weighted_terms(L, S, size, [(([c],), w, float(ws)) for c, w, ws in zip(cts, W.T.tolist(), wscales)])
        cres = None if cvals is None else weight_residues(cvals, [S] * G, self.ctx.primes[:L])
        native = getattr(self.be, "scalar_combine", None)
        if native is not None and m <= capi.COMBINE_MAX_IN and G <= capi.COMBINE_MAX_OUT:
            datas = native(L, size, [c.data for c in cts], [c.parms_id() for c in cts], wres, cres)
        else:
            datas = [self._combine_composed(L, size, [], cts, None, wres[g], None if cres is None else cres[g]) for g in range(G)]
        return [Ciphertext()._set(d, size, L, S) for d in datas]

    def product_combine(self, products, lin=(), const: Optional[float] = None, scale: Optional[float] = None,
                        parms_id: Optional[int] = None) -> List[Ciphertext]:
        """A node of a polynomial plan with its products still inside, for n items in lockstep:
            out[i] = sum_p coef_p * (a_p[i] * b_p[i]) + sum_k coef_k * ct_k[i] + const,
        size 3 and NOT relinearised -- relinearisation is linear, so the caller relinearises the sum once instead of every
        product.  products: (a, b, coef, wscale) with a and b lists of n size-2 ciphertexts (a[i] is b[i] for a square); lin:
        (cts, coef, wscale) with cts a list of n size-2 ciphertexts; the weight of a term is the scalar plaintext
        encode(coef, wscale).  Level parms_id (default: the lowest level among the operands; higher operands are read through
        their row prefix) and scale S: a.scale * b.scale * wscale and ct.scale * wscale must be S for every term -- S is `scale`
        when given, else the first product's; const is encoded at S.
        The words and the checks of the op-by-op sequence -- mod_switch_to, multiply per product, encode and multiply_plain per
        term, add_many, add, add_plain -- from ONE pass over the operands where the backend has hefx_product_combine, else
        from that sequence."""
        products = [(list(a), list(b), float(cf), float(ws)) for a, b, cf, ws in products]
        lin = [(list(cts), float(cf), float(ws)) for cts, cf, ws in lin]
        P, m = len(products), len(lin)
        if P < 1:
            raise ValueError("product_combine: need at least one product")
        n = len(products[0][0])
        if n < 1 or any(len(a) != n or len(b) != n for a, b, _, _ in products) or any(len(cts) != n for cts, _, _ in lin):
            raise ValueError("product_combine: every term needs one operand per item")
        everyone = [x for a, b, _, _ in products for x in a + b] + [x for cts, _, _ in lin for x in cts]
        L = int(parms_id) if parms_id is not None else min(x.parms_id() for x in everyone)
        a0, b0, _, ws0 = products[0]
        S = float(scale) if scale is not None else a0[0].scale * b0[0].scale * ws0
        terms = [((a, b), [cf], ws) for a, b, cf, ws in products] + [((cts,), [cf], ws) for cts, cf, ws in lin]
        res = self._weighted_terms(L, S, 2, terms)[0]
        ures, wres = res[:P], res[P:]
        cres = None if const is None else weight_residues([const], [S], self.ctx.primes[:L])[0]
        native = getattr(self.be, "product_combine", None)
        if native is not None and P <= capi.PRODUCT_COMBINE_MAX_PRODUCTS and m <= capi.PRODUCT_COMBINE_MAX_LIN \
                and n <= capi.PRODUCT_COMBINE_MAX_ITEMS and capi.product_combine_words(L, n, P, m) <= capi.PRODUCT_COMBINE_MAX_WORDS:
            datas = native(L, [[a[i].data for a, _, _, _ in products] for i in range(n)], [a[0].parms_id() for a, _, _, _ in products],
                           [[b[i].data for _, b, _, _ in products] for i in range(n)], [b[0].parms_id() for _, b, _, _ in products], ures,
                           [[cts[i].data for cts, _, _ in lin] for i in range(n)], [cts[0].parms_id() for cts, _, _ in lin], wres, cres)
        else:
            datas = [self._combine_composed(L, 2, [(a[i], b[i]) for a, b, _, _ in products], [cts[i] for cts, _, _ in lin],
                                            ures, wres, cres) for i in range(n)]
        return [Ciphertext()._set(d, 3, L, S) for d in datas]

    def _weighted_terms(self, L: int, S: float, size: int, terms) -> np.ndarray:
        """THE check of scalar weights times ciphertexts, or times products of two, summed at level L and scale S.  terms[t] =
        (factors, weights, wscale): factors is (cts,) for a linear term of `size` polynomials or (a, b) for a product of two
        size-2 operands, each a list over the items that run in lockstep; weights are the G scalars of the G outputs, weight g
        the scalar plaintext encode(weights[g], wscale).  Term by term and item by item, in the order of the op-by-op sequence
        (mod_switch_to, multiply, encode, multiply_plain, add_many): level not below L; size; one level per factor; the bounds
        of the product's scale, of wscale and of the term's scale; closeness to S.  Then S itself, then transparency output by
        output.  Returns the residues of the weights, [G][len(terms)][L]."""
        check_scale = self._check_scale
        for factors, _, ws in terms:
            a, b = factors[0], factors[-1]   # (a linear term: its one factor stands in both places)
            product = len(factors) == 2
            need, size_text = (2, "multiply: only size-2 operands are supported (all reference call sites)") if product \
                else (size, "add_many: mixed sizes are not supported by the fused reduction")
            la, lb = a[0]._parms_id, b[0]._parms_id
            for x, y in zip(a, b):
                if x._parms_id < L or y._parms_id < L:
                    raise ValueError("cannot switch to higher level modulus")
                if x._size != need or y._size != need:
                    raise ValueError(size_text)
                if x._parms_id != la or y._parms_id != lb:
                    raise ValueError("encrypted1 and encrypted2 parameter mismatch")
                s = x._scale
                if product:
                    s = s * y._scale
                    check_scale(s, L)
                check_scale(ws, L)
                check_scale(s * ws, L)
                if not self._close(S, s * ws):
                    raise ValueError("scale mismatch")
        self._check_scale(S, L)
        G = len(terms[0][1])
        for g in range(G):
            for _, w, ws in terms:
                if _c_round(w[g] * ws) == 0:
                    raise RuntimeError("result ciphertext is transparent")  # multiply_plain by the zero plaintext
        flat = weight_residues([w[g] for g in range(G) for _, w, _ in terms], [ws for _, _, ws in terms] * G, self.ctx.primes[:L])
        return flat.reshape(G, len(terms), L)

    def _combine_composed(self, L, size, pairs, lins, ures, wres, cres):
        """one output of scalar_combine (no pairs) or one item of product_combine op by op: mod_drop, multiply, multiply_plain
        by the constant polynomial of each weight at size 3 / `size`, add_many per size, the sum of the linear terms added
        into the first polynomials of the products' sum, add_plain"""
        N, be = self.ctx.N, self.be
        const_poly = lambda res: be.from_host(np.repeat(np.asarray(res, dtype=np.uint64)[:, None], N, axis=1))
        low = lambda x: x.data if x.parms_id() == L else be.mod_drop(x.parms_id(), L, x.size(), x.data)
        total = lambda sz, terms: terms[0] if len(terms) == 1 else be.add_many(L, sz, terms)
        tensor = lambda a, b: be.square(L, low(a)) if a.data is b.data else be.multiply(L, low(a), low(b))
        acc = total(3, [be.multiply_plain(L, 3, tensor(a, b), const_poly(ures[p])) for p, (a, b) in enumerate(pairs)]) if pairs else None
        if lins:
            lin = total(size, [be.multiply_plain(L, size, low(x), const_poly(wres[k])) for k, x in enumerate(lins)])
            acc = lin if acc is None else self._addsub(Ciphertext()._set(acc, 3, L, 1.0), Ciphertext()._set(lin, size, L, 1.0), False).data
        if cres is not None:
            acc = be.add_plain(L, 3 if pairs else size, acc, const_poly(cres))
        return acc

    def mod_raise(self, ct: Ciphertext, parms_id: Optional[int] = None) -> Ciphertext:
        """The first step of CKKS bootstrapping: both polynomials of ct, taken as integer polynomials with centred
        coefficients below its level's modulus Q, written mod the primes of level parms_id (default: the first level).  The
        result decrypts to m + Q * I for a small integer polynomial I (about sqrt((h + 1) / 12) per coefficient for a secret
        key of Hamming weight h); the scale is unchanged.  hefx_mod_raise with count = 2 where the backend has it, else
        ntt_inverse, lift_coefficients and ntt_forward of the new rows.  N <= 16384 (the range of hefx_mod_raise)."""
        L_in = ct.parms_id()
        L_out = int(parms_id) if parms_id is not None else self.ctx.first_parms_id()
        if ct.size() != 2:
            raise ValueError("encrypted size must be 2")
        if L_out < L_in or L_out > self.ctx.first_parms_id():
            raise ValueError("mod_raise: the target level must lie between the ciphertext's and the first level")
        if self.ctx.N > 16384:
            raise ValueError("mod_raise: poly_modulus_degree above 16384 is not supported (the range of hefx_mod_raise)")
        if L_out == L_in:
            return ct.copy()
        be, N = self.be, self.ctx.N
        native = getattr(be, "mod_raise", None)
        if native is not None:
            data = native(L_in, L_out, ct.data, 2)
        else:
            old = np.array(be.to_host(ct.data), dtype=np.uint64).reshape(2, L_in, N)
            coef = np.asarray(be.to_host(be.ntt_inverse(be.from_host(old), 2, L_in, 0))).reshape(2, L_in, N)
            new = np.stack([lift_coefficients(coef[p], self.ctx.primes, L_in, L_out) for p in range(2)])
            new = np.asarray(be.to_host(be.ntt_forward(be.from_host(new), 2, L_out - L_in, L_in))).reshape(2, L_out - L_in, N)
            data = be.from_host(np.concatenate([old, new], axis=1))
        return Ciphertext()._set(data, 2, L_out, ct.scale)

    # ---- hybrid key switching (include/hefx_hybrid.h)
    def _hybrid_level(self, ct: Ciphertext, keys: "HybridKeys") -> int:
        L, top = ct.parms_id(), self.ctx.k - keys.alpha
        if L > top:
            raise ValueError(f"hybrid key switching with alpha = {keys.alpha} needs a ciphertext at a level <= k - alpha = {top}: "
                             f"this one is at level {L} (the last alpha primes of the chain are special primes)")
        return L

    def _hybrid_galois(self, L: int, data, elt: int, keys: "HybridKeys"):
        """(pi_g(c0) + ks0(pi_g(c1)), ks1(pi_g(c1))): hefx_hybrid_apply_galois_batch, or the statement in Python integers"""
        key = keys.hybrid_key(elt)
        native = getattr(self.be, "hybrid_apply_galois_batch", None)
        if native is not None:
            return native(keys.alpha, L, [data], [elt], [key])[0]
        from . import galois_tables
        be, N, q = self.be, self.ctx.N, self.ctx.primes
        ct = np.asarray(be.to_host(data), dtype=np.uint64).reshape(2, L, N)[:, :, galois_tables.gather_table(N, elt)]
        return be.from_host(_hybrid_rows_add_host(q, hybrid_switch_host(be, q, keys.alpha, L, ct[1], be.to_host(key)), ct[:1]))

    def _hybrid_relinearize(self, L: int, data, keys: "HybridKeys"):
        """(c0 + ks0(c2), c1 + ks1(c2)): hefx_hybrid_relinearize_batch, or the statement in Python integers"""
        native = getattr(self.be, "hybrid_relinearize_batch", None)
        if native is not None:
            return native(keys.alpha, L, [data], keys.hybrid_key(0))[0]
        be, N, q = self.be, self.ctx.N, self.ctx.primes
        ct = np.asarray(be.to_host(data), dtype=np.uint64).reshape(3, L, N)
        return be.from_host(_hybrid_rows_add_host(q, hybrid_switch_host(be, q, keys.alpha, L, ct[2], be.to_host(keys.hybrid_key(0))), ct[:2]))

    # ---- hoisted hybrid key switching (include/hefx_hybrid_hoist.h)
    def _hybrid_hoist_args(self, name: str, cts: Sequence[Ciphertext], steps: Sequence[int], keys: "HybridKeys", identity: bool):
        """the common checks of the two hoisted methods -> (L, elts, device keys): one level (the rule of _hybrid_level) and
        size 2; every non-zero step needs its direct key; a step of zero is the identity term (element 1, no key) where
        `identity` says the entry has one, else it is left out"""
        if not isinstance(keys, HybridKeys):
            raise TypeError(f"{name}: needs HybridKeys (KeyGenerator.hybrid_galois_keys)")
        if not cts or not len(steps):
            raise ValueError(f"{name}: need at least one ciphertext and one step")
        L = cts[0].parms_id()
        for c in cts:
            if c.parms_id() != L:
                raise ValueError("encrypted1 and encrypted2 parameter mismatch")
            if c.size() != 2:
                raise ValueError("encrypted size must be 2")
            self._hybrid_level(c, keys)
        elts, dev = [], []
        for s in steps:
            if s == 0 and not identity:
                continue
            elt = 1 if s == 0 else galois_elt_from_step(int(s), self.ctx.N)
            if s != 0 and not keys.has_key(elt):
                raise ValueError("Galois key not present")
            elts.append(elt)
            dev.append(None if s == 0 else keys.hybrid_key(elt))
        if len(cts) * max(len(elts), 1) > capi.HYBRID_HOIST_MAX_TERMS:
            raise ValueError(f"{name}: more than {capi.HYBRID_HOIST_MAX_TERMS} terms (ciphertexts times steps)")
        return L, elts, dev

    def rotate_hoisted(self, cts: Sequence[Ciphertext], steps: Sequence[int], hybrid_keys: "HybridKeys") -> List[List[Ciphertext]]:
        """out[i][k] = cts[i] rotated by steps[k] with ONE digit decomposition per input (hefx_hybrid_rotate_hoisted_batch, or
        the statement in Python integers); a step of zero is a copy.  The ciphertexts share a level <= k - alpha; every
        non-zero step needs its direct key.  NOT the words of rotate_vector with the same keys: the decomposition is
        permuted, not the operand (include/hefx_hybrid_hoist.h) -- the same plaintext and the same noise bound."""
        cts, steps = list(cts), [int(s) for s in steps]
        L, elts, dev = self._hybrid_hoist_args("rotate_hoisted", cts, steps, hybrid_keys, False)
        datas = []
        if elts:
            native = getattr(self.be, "hybrid_rotate_hoisted_batch", None)
            if native is not None:
                datas = native(hybrid_keys.alpha, L, [c.data for c in cts], elts, dev)
            else:
                be, N = self.be, self.ctx.N
                host = [np.asarray(be.to_host(c.data), dtype=np.uint64).reshape(2, L, N) for c in cts]
                datas = [be.from_host(w) for w in hybrid_hoist_host(be, self.ctx.primes, hybrid_keys.alpha, L, host, elts,
                                                                    [be.to_host(k) for k in dev])]
        out, m = [], len(elts)
        for i, c in enumerate(cts):
            moved = iter(datas[i * m:(i + 1) * m])
            out.append([c.copy() if s == 0 else Ciphertext()._set(next(moved), 2, L, c.scale) for s in steps])
        return out

    def plain_combine_hoisted(self, cts: Sequence[Ciphertext], steps: Sequence[int], rows: Sequence[Sequence[Optional[Plaintext]]],
                              hybrid_keys: "HybridKeys") -> List[Ciphertext]:
        """Double hoisting on hybrid keys: out[o] = sum over i, k of rows[o][i * len(steps) + k] (.) rotate(cts[i], steps[k]) over
        the entries that are not None, with ONE digit decomposition per input and ONE mod-down per output
        (hefx_hybrid_plain_combine_hoisted, or the statement in Python integers).  The plaintexts are KEY-LEVEL plaintexts
        (encode with parms_id = k) of one scale; a step of zero is the identity term and needs no key.  The checks are those
        of plain_combine, plus the level rule of hybrid key switching; a missing key is a ValueError.  The scale is the
        product of the operand scales.  One rounding per output: not the words of rotate_vector + multiply_plain + add_many."""
        cts, steps, rows = list(cts), [int(s) for s in steps], [list(r) for r in rows]
        L, elts, dev = self._hybrid_hoist_args("plain_combine_hoisted", cts, steps, hybrid_keys, True)
        terms = len(cts) * len(steps)
        if not rows or any(len(r) != terms for r in rows):
            raise ValueError("plain_combine_hoisted: need one plaintext (or None) per output, ciphertext and step")
        if len(rows) > capi.HYBRID_HOIST_MAX_OUT:
            raise ValueError(f"plain_combine_hoisted: more than {capi.HYBRID_HOIST_MAX_OUT} outputs")
        ct_scale = cts[0].scale
        if any(not self._close(ct_scale, c.scale) for c in cts):
            raise ValueError("scale mismatch")
        if any(all(p is None for p in r) for r in rows):
            raise ValueError("plain_combine_hoisted: an output has no term")
        scale = self._plain_product_scale(L, ct_scale, [p for r in rows for p in r if p is not None], self.ctx.k)
        native = getattr(self.be, "hybrid_plain_combine_hoisted", None)
        if native is not None:
            datas = native(hybrid_keys.alpha, L, [c.data for c in cts], elts, dev, [[None if p is None else p.data for p in r] for r in rows])
        else:
            be, N = self.be, self.ctx.N
            host = [np.asarray(be.to_host(c.data), dtype=np.uint64).reshape(2, L, N) for c in cts]
            datas = [be.from_host(w) for w in hybrid_hoist_host(
                be, self.ctx.primes, hybrid_keys.alpha, L, host, elts, [None if k is None else be.to_host(k) for k in dev],
                [[None if p is None else be.to_host(p.data) for p in r] for r in rows])]
        return [Ciphertext()._set(d, 2, L, scale) for d in datas]

    def bsgs_hoisted(self, cts: Sequence[Ciphertext], baby_steps: Sequence[int], rows: Sequence[Sequence[Optional[Plaintext]]],
                     giant_steps: Sequence[int], dest: Sequence[int], hybrid_keys: "HybridKeys") -> List[Ciphertext]:
        """A baby-step giant-step stage on hybrid keys in one call, the giant steps hoisted too: inner sum o is
        plain_combine_hoisted's rows[o] over cts and baby_steps, kept in the extended basis; it is rotated by giant_steps[o]
        (0: no rotation) and added into output dest[o]; every output takes ONE mod-down (hefx_hybrid_bsgs_hoisted, or the
        statement in Python integers).  rows: key-level plaintexts of one scale, as in plain_combine_hoisted, whose checks
        hold here; also a ValueError: a giant step without its key, a dest outside 0 .. max(dest), an output that no inner sum
        feeds.  Not the words of plain_combine_hoisted + rotate_vector + add_many: those round every inner sum and every
        giant rotation, this rounds c1 of an inner sum once and every output once."""
        cts, steps, rows = list(cts), [int(s) for s in baby_steps], [list(r) for r in rows]
        giant_steps, dest = [int(s) for s in giant_steps], [int(d) for d in dest]
        L, elts, dev = self._hybrid_hoist_args("bsgs_hoisted", cts, steps, hybrid_keys, True)
        terms = len(cts) * len(steps)
        if not rows or any(len(r) != terms for r in rows):
            raise ValueError("bsgs_hoisted: need one plaintext (or None) per inner sum, ciphertext and step")
        if len(rows) > capi.HYBRID_HOIST_MAX_OUT:
            raise ValueError(f"bsgs_hoisted: more than {capi.HYBRID_HOIST_MAX_OUT} inner sums")
        ct_scale = cts[0].scale
        if any(not self._close(ct_scale, c.scale) for c in cts):
            raise ValueError("scale mismatch")
        if any(all(p is None for p in r) for r in rows):
            raise ValueError("bsgs_hoisted: an inner sum has no term")
        if len(giant_steps) != len(rows) or len(dest) != len(rows):
            raise ValueError("bsgs_hoisted: need one giant step and one dest per inner sum")
        O = max(dest) + 1
        if min(dest) < 0 or O > len(rows):
            raise ValueError("bsgs_hoisted: dest out of range")
        if set(dest) != set(range(O)):
            raise ValueError("bsgs_hoisted: an output has no inner sum")
        gelts = [1 if s == 0 else galois_elt_from_step(s, self.ctx.N) for s in giant_steps]
        if any(s != 0 and not hybrid_keys.has_key(e) for s, e in zip(giant_steps, gelts)):
            raise ValueError("Galois key not present")
        gdev = [None if s == 0 else hybrid_keys.hybrid_key(e) for s, e in zip(giant_steps, gelts)]
        scale = self._plain_product_scale(L, ct_scale, [p for r in rows for p in r if p is not None], self.ctx.k)
        native = getattr(self.be, "hybrid_bsgs_hoisted", None)
        if native is not None:
            datas = native(hybrid_keys.alpha, L, [c.data for c in cts], elts, dev, [[None if p is None else p.data for p in r] for r in rows],
                           gelts, gdev, dest)
        else:
            be, N = self.be, self.ctx.N
            host = [np.asarray(be.to_host(c.data), dtype=np.uint64).reshape(2, L, N) for c in cts]
            cache = {}  # a giant key is read by every output's inner sum of its step: brought to the host once

            def to_host(key):
                if key is not None and id(key) not in cache:
                    cache[id(key)] = be.to_host(key)
                return None if key is None else cache[id(key)]
            datas = [be.from_host(w) for w in hybrid_bsgs_host(
                be, self.ctx.primes, hybrid_keys.alpha, L, host, elts, [to_host(k) for k in dev],
                [[None if p is None else be.to_host(p.data) for p in r] for r in rows], gelts, [to_host(k) for k in gdev], dest)]
        return [Ciphertext()._set(d, 2, L, scale) for d in datas]

    def apply_galois(self, a: Ciphertext, galois_elt: int, galois_keys: KSwitchKeys, destination=None):
        """Evaluator::apply_galois: the automorphism X -> X^galois_elt and the key switch back, with the key of that element"""
        if a.size() != 2:
            raise ValueError("encrypted size must be 2")
        if not galois_keys.has_key(galois_elt):
            raise ValueError("Galois key not present")
        L = a.parms_id()
        if isinstance(galois_keys, HybridKeys):
            data = self._hybrid_galois(self._hybrid_level(a, galois_keys), a.data, galois_elt, galois_keys)
        else:
            data = self.be.apply_galois(L, a.data, galois_elt, galois_keys.key(galois_elt))
        out = destination if destination is not None else Ciphertext()
        return out._set(data, 2, L, a.scale)

    def switch_key(self, ct: Ciphertext, key) -> Ciphertext:
        """(c0 + ks0(c1), ks1(c1)) with a switching key [k-1][2][k][N] from the secret ct is under to another one: the key
        switch of a rotation without its automorphism.  Size 2, any level.  hefx_switch_key where the backend has it, else
        its apply_galois with the Galois element 1 -- the same words."""
        if ct.size() != 2:
            raise ValueError("encrypted size must be 2")
        L = ct.parms_id()
        if isinstance(key, HybridKeys):  # the hybrid key under the identity element (KeyGenerator.hybrid_switching_key)
            if not key.has_key(1):
                raise ValueError("switch_key: the HybridKeys hold no key under the identity element 1")
            return Ciphertext()._set(self._hybrid_galois(self._hybrid_level(ct, key), ct.data, 1, key), 2, L, ct.scale)
        native = getattr(self.be, "switch_key", None)
        data = native(L, ct.data, key) if native is not None else self.be.apply_galois(L, ct.data, 1, key)
        return Ciphertext()._set(data, 2, L, ct.scale)

    def raise_switch(self, ct: Ciphertext, keys: "EncapsKeys", parms_id: Optional[int] = None) -> Ciphertext:
        """Mod-raise under the sparse secret and switch back to the main one, as one step: ct, a size-2 ciphertext at the last
        prime q_0 under the auxiliary secret of `keys` (switch_key(., keys.low)), comes back at level parms_id (default: the
        first level) under the main secret, decrypting to m + q_0 I with the I of the SPARSE secret.  x, the centred lift of
        c1, has |x| < q_0 / 2 -- one digit -- so the switch is moddown(x * Kc) with the collapsed key Kc = sum of the
        digits of keys.high: 4 L + 3 row transforms where mod_raise + switch_key take about L^2 + 5 L.  The scale is
        unchanged.  Any N the engine serves, 32768 included.

        hefx_raise_switch where the backend has it (the collapsed key is cached on `keys` per level).  Otherwise the
        REFERENCE: the backend's ordinary apply_galois(L, ., 1, .) on a synthetic two-digit operand -- x = c1 - q_0 neg,
        neg the 0/1 polynomial of the coefficients above q_0 // 2, as target rows (c1's row, NTT_q1(neg), zeros) against
        the key (Kc, (-q_0 mod q_m) Kc, zeros) -- so that every modulus sees x Kc: the same words by exact modular
        arithmetic, with the lift of c0 (lift_coefficients) as the c0 the key switch adds to.

        keys may be the HybridEncapsKeys of KeyGenerator.hybrid_encapsulation_keys: the same step on hybrid keys, to a level in
        2 .. k - alpha (default k - alpha): _hybrid_raise_switch."""
        if ct.size() != 2:
            raise ValueError("encrypted size must be 2")
        if ct.parms_id() != 1:
            raise ValueError("raise_switch: needs a ciphertext at the last prime")
        if isinstance(keys, HybridEncapsKeys):
            return self._hybrid_raise_switch(ct, keys, parms_id)
        L = int(parms_id) if parms_id is not None else self.ctx.first_parms_id()
        if L < 2 or L > self.ctx.first_parms_id():
            raise ValueError("raise_switch: the target level must lie between 2 and the first level")
        be, N, k, q = self.be, self.ctx.N, self.ctx.k, [int(p) for p in self.ctx.primes]
        native, collapse = getattr(be, "raise_switch", None), getattr(be, "collapse_key", None)
        if native is not None and collapse is not None:
            ckey = keys._collapsed.get(L)
            if ckey is None:
                ckey = keys._collapsed[L] = collapse(L, keys.high)
            return Ciphertext()._set(native(L, ct.data, ckey), 2, L, ct.scale)
        return Ciphertext()._set(self._raise_switch_composed(ct, keys, L), 2, L, ct.scale)

    def _hybrid_raise_switch(self, ct: Ciphertext, keys: "HybridEncapsKeys", parms_id: Optional[int]) -> Ciphertext:
        """raise_switch with KeyGenerator.hybrid_encapsulation_keys (include/ext/hefx_hybrid_encaps.h): the target level lies in
        2 .. k - alpha (default k - alpha, the top of a hybrid program); 4 L + 3 alpha row transforms.  hefx_hybrid_raise_switch
        with the collapsed key cached on `keys` per level where the backend has it, otherwise hybrid_raise_switch_host: the
        same words."""
        alpha, top = keys.high.alpha, self.ctx.k - keys.high.alpha
        L = int(parms_id) if parms_id is not None else top
        if L < 2 or L > top:
            raise ValueError(f"raise_switch: with alpha = {alpha} the target level must lie between 2 and k - alpha = {top}")
        be, q = self.be, self.ctx.primes
        native, collapse = getattr(be, "hybrid_raise_switch", None), getattr(be, "hybrid_collapse_key", None)
        ckey = keys._collapsed.get(L)
        if native is not None and collapse is not None:
            if ckey is None:
                ckey = keys._collapsed[L] = collapse(alpha, L, keys.high.hybrid_key(1))
            return Ciphertext()._set(native(alpha, L, ct.data, ckey), 2, L, ct.scale)
        if ckey is None:
            ckey = keys._collapsed[L] = hybrid_collapse_key_host(be.to_host(keys.high.hybrid_key(1)), q, alpha, L)
        return Ciphertext()._set(be.from_host(hybrid_raise_switch_host(be, q, alpha, L, be.to_host(ct.data), ckey)), 2, L, ct.scale)

    def _raise_switch_composed(self, ct: Ciphertext, keys: "EncapsKeys", L: int):
        """raise_switch's words from the backend's ordinary key switch (the reference form its docstring states)"""
        be, N, k, q = self.be, self.ctx.N, self.ctx.k, [int(p) for p in self.ctx.primes]
        old = np.array(be.to_host(ct.data), dtype=np.uint64).reshape(2, 1, N)
        coef = np.asarray(be.to_host(be.ntt_inverse(be.from_host(old), 2, 1, 0))).reshape(2, N)
        target = np.zeros((2, L, N), dtype=np.uint64)
        target[:, 0] = old[:, 0]
        lifted = be.ntt_forward(be.from_host(lift_coefficients(coef[0][None], q, 1, L)), 1, L - 1, 1)
        target[0, 1:] = np.asarray(be.to_host(lifted)).reshape(L - 1, N)
        neg = (coef[1] > np.uint64(q[0] // 2)).astype(np.uint64)
        target[1, 1] = np.asarray(be.to_host(be.ntt_forward(be.from_host(neg[None, None]), 1, 1, 1))).reshape(N)
        kc = collapse_key_host(be.to_host(keys.high), q, L)
        synth = np.zeros((k - 1, 2, k, N), dtype=np.uint64)
        synth[0] = kc
        for m in range(k):
            synth[1][:, m] = (kc[:, m].astype(object) * ((-q[0]) % q[m]) % q[m]).astype(np.uint64)
        return be.apply_galois(L, be.from_host(target), 1, be.from_host(synth))

    def plain_combine(self, cts: Sequence[Ciphertext], pts_matrix: Sequence[Sequence[Optional[Plaintext]]]) -> List[Ciphertext]:
        """G plaintext combinations of the same ciphertexts: out[g] = sum_k pts_matrix[g][k] (.) cts[k] over the entries that
        are not None (None: a structural zero, no term) -- the inner sums of a baby-step/giant-step matrix product, all giant
        steps at once.  The ciphertexts share one level and scale and so do the plaintexts; the result's scale is their
        product.  The words and the checks of multiply_plain per term and add_many, from ONE pass over the inputs where the
        backend has hefx_plain_combine (small uniform shapes: from one grouped multiply_plain_sum, see below), else from
        multiply_plain_sum per output."""
        cts = list(cts)
        rows = [list(r) for r in pts_matrix]
        m = len(cts)
        if m < 1 or not rows or any(len(r) != m for r in rows):
            raise ValueError("plain_combine: need one plaintext (or None) per output and ciphertext")
        L, size, ct_scale = cts[0].parms_id(), cts[0].size(), cts[0].scale
        for c in cts:
            if c.parms_id() != L:
                raise ValueError("encrypted1 and encrypted2 parameter mismatch")
            if c.size() != 2 or size != 2:
                raise ValueError("encrypted size must be 2")
            if not self._close(ct_scale, c.scale):
                raise ValueError("scale mismatch")
        if any(all(p is None for p in r) for r in rows):
            raise ValueError("plain_combine: an output has no term")
        scale = self._plain_product_scale(L, ct_scale, [p for r in rows for p in r if p is not None], L)
        counts = [sum(p is not None for p in r) for r in rows]
        route = capi.plain_combine_route(getattr(self.be, "plain_combine", None) is not None, m, counts, L * self.ctx.N)
        if route == "grouped":
            datas = self.be.multiply_plain_sum(L, 2, [c.data for r in rows for c, p in zip(cts, r) if p is not None],
                                               [p.data for r in rows for p in r if p is not None], counts[0])
        elif route == "fused":
            datas = self.be.plain_combine(L, [c.data for c in cts], [[None if p is None else p.data for p in r] for r in rows])
        else:
            datas = [self.be.multiply_plain_sum(L, 2, [c.data for c, p in zip(cts, r) if p is not None],
                                                [p.data for p in r if p is not None])[0] for r in rows]
        return [Ciphertext()._set(d, 2, L, scale) for d in datas]

    def multiply_sum(self, As: Sequence[Ciphertext], Bs: Sequence[Ciphertext], group: Optional[int] = None):
        """add_many(multiply(As[i], Bs[i])) per group of `group` consecutive terms (None: one group) in one pass over
        the operands (hefx_multiply_sum): the products and the sum of Linear_Transform_Cipher (helper.h:222-231) and
        sum_k A_k * B_k (matrix_multiplication.cpp:123-129).  The size-3 sums are not relinearised.  Checks, messages and
        their order are those of the op-by-op sequence -- per group every multiply, then add_many -- and so are the bits.
        Returns the list of group sums."""
        if not As or len(As) != len(Bs):
            raise ValueError("multiply_sum: need as many second operands as first operands")
        n = len(As)
        group = n if group is None else int(group)
        if group < 1:
            raise ValueError("multiply_sum: group must be positive")
        heads = []
        for g0 in range(0, n, group):
            terms = list(zip(As[g0:g0 + group], Bs[g0:g0 + group]))
            for a, b in terms:                                       # Evaluator::multiply, term by term
                self._check_same(a, b)
                if a.size() != 2 or b.size() != 2:
                    raise ValueError("multiply: only size-2 operands are supported (all reference call sites)")
                self._check_scale(a.scale * b.scale, a.parms_id())
            a0, b0 = terms[0]
            for a, b in terms[1:]:                                   # Evaluator::add_many over the group's products
                if a.parms_id() != a0.parms_id():
                    raise ValueError("encrypted1 and encrypted2 parameter mismatch")
                if not self._close(a0.scale * b0.scale, a.scale * b.scale):
                    raise ValueError("scale mismatch")
            heads.append((a0.parms_id(), a0.scale * b0.scale))
        f = getattr(self.be, "multiply_sum", None)
        if f is None or any(L != heads[0][0] for L, _ in heads):     # no fused sum (or groups at different levels)
            return [self.add_many([self.multiply(a, b) for a, b in zip(As[g0:g0 + group], Bs[g0:g0 + group])])
                    for g0 in range(0, n, group)]
        L = heads[0][0]
        outs = f(L, [a.data for a in As], [b.data for b in Bs], group)
        return [Ciphertext()._set(o, 3, L, s) for o, (_, s) in zip(outs, heads)]

    def multiply(self, a: Ciphertext, b: Ciphertext, destination=None):
        """Evaluator::multiply for ciphertexts of any size: the result has size(a) + size(b) - 1 polynomials and is not
        relinearised.  Size 2 x size 2 goes to the engine's dedicated kernels, any other shape to hefx_multiply_sizes."""
        self._check_same(a, b)
        sa, sb = a.size(), b.size()
        general = getattr(self.be, "multiply_sizes", None) if (sa, sb) != (2, 2) else None
        if (sa, sb) != (2, 2) and general is None:
            raise ValueError("multiply: only size-2 operands are supported (all reference call sites)")
        if sa < 2 or sb < 2 or sa + sb - 1 > CT_SIZE_MAX:
            raise ValueError("invalid size")  # SEAL: Ciphertext::resize refuses the destination
        new_scale = a.scale * b.scale
        self._check_scale(new_scale, a.parms_id())
        L = a.parms_id()
        if general is not None:
            data = general(L, sa, a.data, sb, b.data)
        else:
            data = self.be.square(L, a.data) if a.data is b.data else self.be.multiply(L, a.data, b.data)
        out = destination if destination is not None else Ciphertext()
        return out._set(data, sa + sb - 1, L, new_scale)

    def multiply_inplace(self, a, b):
        return self.multiply(a, b, a)

    def square(self, a, destination=None):
        return self.multiply(a, a, destination)

    def square_inplace(self, a):
        return self.multiply(a, a, a)

    # ---- relinearize / rescale / mod switch
    def relinearize_inplace(self, a: Ciphertext, relin_keys: KSwitchKeys):
        if a.size() == 2:
            return a  # SEAL: nothing to do (true at logistic_regression_ckks.cpp:237,319)
        if a.size() == 3:
            if not relin_keys.has_key(0):
                raise ValueError("not enough relinearization keys")
            if isinstance(relin_keys, HybridKeys):
                return a._set(self._hybrid_relinearize(self._hybrid_level(a, relin_keys), a.data, relin_keys), 2, a.parms_id(), a.scale)
            return a._set(self.be.relinearize(a.parms_id(), a.data, relin_keys.key(0)), 2, a.parms_id(), a.scale)
        if isinstance(relin_keys, HybridKeys):
            relin_keys._refuse()
        # any larger size: SEAL's relinearize_internal -- from the top, polynomial t with the key of s^t into (c0, c1)
        general = getattr(self.be, "relinearize_sizes", None)
        if general is None or a.size() < 2:
            raise ValueError("relinearize: encrypted size must be 2 or 3")
        if a.size() > CT_SIZE_MAX:
            raise ValueError("encrypted is not valid for encryption parameters")
        if not all(relin_keys.has_power(p) for p in range(2, a.size())):
            raise ValueError("not enough relinearization keys")
        keys = [relin_keys.power_key(p) for p in range(2, a.size())]
        return a._set(general(a.parms_id(), a.size(), 2, a.data, keys), 2, a.parms_id(), a.scale)

    def rescale_to_next_inplace(self, a: Ciphertext):
        L = a.parms_id()
        if L <= 1:
            raise ValueError("end of modulus switching chain reached")
        q_last = self.ctx.primes[L - 1]
        return a._set(self.be.rescale(L, a.size(), a.data), a.size(), L - 1, a.scale / float(q_last))

    def mod_switch_to_next_inplace(self, x):
        return self.mod_switch_to_inplace(x, x.parms_id() - 1)

    def mod_switch_to_inplace(self, x, parms_id: int):
        L = x.parms_id()
        if parms_id > L:
            raise ValueError("cannot switch to higher level modulus")
        if parms_id < 1:
            raise ValueError("end of modulus switching chain reached")
        if parms_id == L:
            return x
        if isinstance(x, Plaintext):
            x.data = self.be.mod_drop(L, parms_id, 1, x.data)
            x._parms_id = parms_id
            return x
        return x._set(self.be.mod_drop(L, parms_id, x.size(), x.data), x.size(), parms_id, x.scale)

    # ---- rotations
    def rotation_plan(self, steps: int, galois_keys: KSwitchKeys) -> List[int]:
        """Galois elements SEAL's rotate_internal applies, in order (App. A.7)."""
        if steps == 0:
            return []
        N = self.ctx.N
        elt = galois_elt_from_step(steps, N)
        if galois_keys.has_key(elt):
            return [elt]
        terms = naf(steps)
        if len(terms) == 1:
            raise ValueError("Galois key not present")
        plan: List[int] = []
        for t in terms:
            if abs(t) == N // 2:
                continue
            plan += self.rotation_plan(t, galois_keys)
        return plan

    def rotate_vector(self, a: Ciphertext, steps: int, galois_keys: KSwitchKeys, destination=None):
        if a.size() != 2:
            raise ValueError("encrypted size must be 2")
        data, L = a.data, a.parms_id()
        hybrid = isinstance(galois_keys, HybridKeys)
        if hybrid:
            self._hybrid_level(a, galois_keys)
        for elt in self.rotation_plan(steps, galois_keys):
            data = self._hybrid_galois(L, data, elt, galois_keys) if hybrid else self.be.apply_galois(L, data, elt, galois_keys.key(elt))
        out = destination if destination is not None else Ciphertext()
        return out._set(data, 2, L, a.scale)

    def rotate_vector_inplace(self, a, steps, galois_keys):
        return self.rotate_vector(a, steps, galois_keys, a)

    def complex_conjugate(self, a: Ciphertext, galois_keys: KSwitchKeys, destination=None):
        """Evaluator::complex_conjugate: the Galois element 2N - 1, every slot conjugated"""
        if a.size() != 2:
            raise ValueError("encrypted size must be 2")
        elt = 2 * self.ctx.N - 1
        if not galois_keys.has_key(elt):
            raise ValueError("Galois key not present")
        if isinstance(galois_keys, HybridKeys):
            data = self._hybrid_galois(self._hybrid_level(a, galois_keys), a.data, elt, galois_keys)
        else:
            data = self.be.apply_galois(a.parms_id(), a.data, elt, galois_keys.key(elt))
        out = destination if destination is not None else Ciphertext()
        return out._set(data, 2, a.parms_id(), a.scale)

    def complex_conjugate_inplace(self, a, galois_keys):
        return self.complex_conjugate(a, galois_keys, a)
