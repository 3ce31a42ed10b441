"""The oracle-backed twin with the general-size routes (TEST INFRASTRUCTURE for tests/test_ct_sizes_cpu.py and
tests/test_gpu_ct_sizes.py): OracleBackend plus multiply_sizes / relinearize_sizes, stated with oracle.Oracle.multiply and
a loop of Oracle.switch_key in the order of SEAL's relinearize_internal.  It has no addsub_unequal: sums of unequal sizes
take the Evaluator's padded form there, which is the statement the engine's device route must equal."""
import numpy as np

from tests.oracle_backend import OracleBackend

VALUES = (np.array([0.5, -1.0, 0.25, 1.0, -0.75, 0.125, 0.9, -0.3]),
          np.array([-0.5, 0.75, 1.0, -1.0, 0.3, 0.6, -0.8, 0.45]),
          np.array([1.0, 0.5, -0.25, -0.6, 0.7, -1.0, 0.2, 0.35]))


class SizesOracleBackend(OracleBackend):
    def multiply_sizes(self, L, size_a, a, size_b, b):
        return self.o.multiply(self._ct(a, size_a, L), self._ct(b, size_b, L))

    def relinearize_sizes(self, L, size_in, size_out, ct, keys):
        c = self._ct(ct, size_in, L)
        head = np.ascontiguousarray(c[:2])
        for t in range(size_in - 1, size_out - 1, -1):
            head = self.o.switch_key(head, c[t], keys[t - 2])
        return np.concatenate([head, c[2:size_out]]) if size_out > 2 else head


def make(N, bits, backend_kind, seed=1, relin_count=2):
    """the environment of tests/test_gpu_composites.make, with the twin above as the "oracle" kind and relin_keys(count)"""
    import os
    from seal_fyp_logistic_regression_amd import seal as S
    parms = S.EncryptionParameters("ckks")
    parms.set_poly_modulus_degree(N)
    parms.set_coeff_modulus(S.CoeffModulus.Create(N, bits))
    backend = {"oracle": SizesOracleBackend, "plain_oracle": OracleBackend}.get(backend_kind)
    ctx = S.SEALContext.Create(parms, backend=backend(N, parms.coeff_modulus()) if backend else None)
    assert ctx.backend.rescale_rounded == (os.environ.get("HEFX_RESCALE", "round") != "floor"), backend_kind
    kg = S.KeyGenerator(ctx, seed)
    return dict(ctx=ctx, kg=kg, enc=S.Encryptor(ctx, kg.public_key(), seed + 1), dec=S.Decryptor(ctx, kg.secret_key()),
                encoder=S.CKKSEncoder(ctx, device_encode=False), ev=S.Evaluator(ctx), rk=kg.relin_keys(relin_count))


def xyz(e, scale=2.0 ** 30):
    """x * y * z without intermediate relinearisation (size 4), one relinearize_inplace, two rescales"""
    ev = e["ev"]
    x, y, z = (e["enc"].encrypt(e["encoder"].encode(v, scale)) for v in VALUES)
    size4 = ev.multiply(ev.multiply(x, y), z)
    relin = size4.copy()
    ev.relinearize_inplace(relin, e["rk"])
    rescaled = relin.copy()
    ev.rescale_to_next_inplace(rescaled)
    ev.rescale_to_next_inplace(rescaled)
    return dict(size4=size4, relin=relin, rescaled=rescaled)
