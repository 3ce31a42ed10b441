"""The aliasing rule of the C-ABI as data (TEST INFRASTRUCTURE): one row per entry of include/hefx.h that takes device
inputs and writes a device output -- what it serves in place, what it refuses, and the test that holds it to that.
tests/test_aliasing_cpu.py requires a row for every such declaration; tests/test_gpu_aliasing.py runs the rows whose
`test` lies in that file on the GPU.  INTEGRATION.md ("Aliasing") prints the same table for the integrator.

Kinds
  IN_PLACE    the output may BE an operand, exactly (same start, same size); any other shared byte is refused
  IN_PLACE_SUM  hefx_add_many: the output may be any of the inputs, repeated pointers included
  NO_OVERLAP  no output shares a byte with an input of the call or with another output; HEFX_ERR_INVALID before anything
              is submitted; adjacent views are fine
  UNCHANGED   the entry had a stated, tested rule before this table was written; `test` names that test
"""

IN_PLACE, IN_PLACE_SUM, NO_OVERLAP, UNCHANGED = "in place", "in place (sum)", "no overlap", "unchanged"

G = "tests/test_gpu_aliasing.py"


def _row(kind, serves, refuses, test):
    return {"kind": kind, "serves": serves, "refuses": refuses, "test": test}


_EW = ("d_out one row into d_a or d_b", "d_a or d_b one row into d_out")
_LT = ("d_out == d_ct", "d_out one row into a diagonal")

RULES = {
    # ---- exact in place allowed, any other overlap refused
    "hefx_add": _row(IN_PLACE, ("d_out == d_a", "d_out == d_b", "d_out == d_a == d_b"), _EW, f"{G}::test_elementwise_in_place"),
    "hefx_sub": _row(IN_PLACE, ("d_out == d_a", "d_out == d_b"), _EW, f"{G}::test_elementwise_in_place"),
    "hefx_negate": _row(IN_PLACE, ("d_out == d_a",), ("d_out one row into d_a", "d_a one row into d_out"),
                        f"{G}::test_elementwise_in_place"),
    "hefx_add_plain": _row(IN_PLACE, ("d_out == d_ct",), ("d_out one row into d_ct", "d_out on d_pt"),
                           f"{G}::test_elementwise_in_place"),
    "hefx_multiply_plain": _row(IN_PLACE, ("d_out == d_ct",), ("d_out one row into d_ct", "d_out on d_pt"),
                                f"{G}::test_elementwise_in_place"),
    "hefx_add_batch": _row(IN_PLACE, ("d_out[i] == d_a[i]", "d_out[i] == d_b[i]", "one shared read-only d_b"),
                           ("d_out[i] == d_a[j]", "two outputs one row apart", "d_out[i] one row into d_b[j]"),
                           f"{G}::test_addsub_batch_in_place"),
    "hefx_sub_batch": _row(IN_PLACE, ("d_out[i] == d_a[i]", "d_out[i] == d_b[i]", "one shared read-only d_b"),
                           ("d_out[i] == d_a[j]", "two outputs one row apart", "d_out[i] one row into d_b[j]"),
                           f"{G}::test_addsub_batch_in_place"),
    "hefx_add_many": _row(IN_PLACE_SUM, ("d_out == d_in[i], any i, any n, repeated pointers included",),
                          ("d_out one row into d_in[i]",), f"{G}::test_add_many_in_place"),
    # ---- no overlap at all
    "hefx_multiply": _row(NO_OVERLAP, (), ("d_out3 == d_a", "d_out3 one row into d_b", "d_a one row into d_out3"), f"{G}::test_refusals"),
    "hefx_square": _row(NO_OVERLAP, (), ("d_out3 == d_a", "d_a one row into d_out3"), f"{G}::test_refusals"),
    "hefx_multiply_batch": _row(NO_OVERLAP, (), ("d_out3[i] == d_a[j]", "two outputs one row apart", "d_b[j] one row into d_out3[i]"),
                                f"{G}::test_refusals"),
    "hefx_multiply_plain_batch": _row(NO_OVERLAP, (), ("d_outs[i] == d_cts[j]", "d_outs[i] on d_pts[j]", "two outputs one row apart"),
                                      f"{G}::test_refusals"),
    "hefx_multiply_plain_sum": _row(NO_OVERLAP, (), ("d_outs[g] == an input of another group", "d_outs[g] on d_pts[i]",
                                                     "two outputs one row apart"), f"{G}::test_refusals"),
    "hefx_rescale_to_next": _row(NO_OVERLAP, (), ("d_out == d_in", "d_out one row into d_in", "d_in one row into d_out"),
                                 f"{G}::test_refusals"),
    "hefx_rescale_to_next_mode": _row(NO_OVERLAP, (), ("d_out == d_in", "d_out one row into d_in", "d_in one row into d_out"),
                                      f"{G}::test_refusals"),
    "hefx_rescale_to_next_batch": _row(NO_OVERLAP, (), ("d_out[i] == d_in[j]", "two outputs one row apart", "d_out[i] one row into d_in[i]"),
                                       f"{G}::test_refusals"),
    "hefx_mod_drop": _row(NO_OVERLAP, (), ("d_out == d_in", "d_out one row into d_in", "d_in one row into d_out"), f"{G}::test_refusals"),
    "hefx_galois_permute": _row(NO_OVERLAP, (), ("d_out == d_in", "d_out one row into d_in", "d_in one row into d_out"),
                                f"{G}::test_refusals"),
    "hefx_decrypt": _row(NO_OVERLAP, (), ("d_out == d_ct", "d_out one row into d_ct", "d_out on d_sk"), f"{G}::test_refusals"),
    "hefx_encrypt": _row(NO_OVERLAP, (), ("d_out == d_plain", "d_out one row into d_pk", "d_plain one row into d_out"),
                         f"{G}::test_refusals"),
    "hefx_encrypt_batch": _row(NO_OVERLAP, (), ("d_outs[i] == d_plains[j]", "two outputs one row apart", "d_outs[i] one row into d_pk"),
                               f"{G}::test_refusals"),
    "hefx_keygen_kswitch": _row(NO_OVERLAP, (), ("d_out one row into d_sk", "d_new_sk one row into d_out"),
                                f"{G}::test_keygen_kswitch_refusals"),
    "hefx_linear_transform_plain": _row(NO_OVERLAP, (), _LT, f"{G}::test_linear_transform_refusals"),
    "hefx_linear_transform_plain_many": _row(NO_OVERLAP, (), _LT + ("two equal outputs",), f"{G}::test_linear_transform_refusals"),
    "hefx_linear_transform_plain_hoisted": _row(NO_OVERLAP, (), _LT, f"{G}::test_linear_transform_refusals"),
    "hefx_linear_transform_plain_hoisted2": _row(NO_OVERLAP, (), _LT, f"{G}::test_linear_transform_refusals"),
    "hefx_linear_transform_plain_hoisted2_sparse": _row(NO_OVERLAP, (), _LT, f"{G}::test_linear_transform_refusals"),
    "hefx_linear_transform_plain_bsgs": _row(NO_OVERLAP, (), _LT, f"{G}::test_linear_transform_refusals"),
    "hefx_rotate_hoisted_batch": _row(NO_OVERLAP, (), ("an output == d_ct_in", "an output one row into a plaintext",
                                                       "n = 1: the output one row into d_ct_in"), f"{G}::test_linear_transform_refusals"),
    # ---- entries whose rule was stated and tested before
    "hefx_multiply_sizes": _row(UNCHANGED, (), ("the output on an input, in bytes",),
                                "tests/test_gpu_ct_sizes.py::test_refusals_come_before_anything_is_written"),
    "hefx_multiply_sizes_batch": _row(UNCHANGED, (), ("any output on any input or output, in bytes",),
                                      "tests/test_gpu_ct_sizes.py::test_refusals_come_before_anything_is_written"),
    "hefx_relinearize_sizes": _row(UNCHANGED, (), ("the output on the input, in bytes",),
                                   "tests/test_gpu_ct_sizes.py::test_refusals_come_before_anything_is_written"),
    "hefx_relinearize_sizes_batch": _row(UNCHANGED, (), ("any output on any input or output, in bytes",),
                                         "tests/test_gpu_ct_sizes.py::test_refusals_come_before_anything_is_written"),
    "hefx_relinearize": _row(NO_OVERLAP, (), ("d_ct2 == d_ct3", "d_ct2 one row into d_ct3", "d_ct3 one row into d_ct2"), f"{G}::test_refusals"),
    "hefx_relinearize_batch": _row(NO_OVERLAP, (), ("d_ct2[i] == d_ct3[j]", "two outputs one row apart"), f"{G}::test_refusals"),
    # ---- the key-switch host path: one check (ks_run's, through csrc/hefx_ranges.h) for every n, the rotations and the sums
    # as one list of 2n outputs
    "hefx_apply_galois": _row(IN_PLACE, ("d_ct_out == d_ct_in",), ("d_ct_out one row into d_ct_in", "d_ct_in one row into d_ct_out"),
                              f"{G}::test_apply_galois_one_item"),
    "hefx_apply_galois_batch": _row(IN_PLACE, ("d_ct_out[i] == d_ct_in[i]",),
                                    ("d_ct_out[1] == d_ct_in[0]", "an input one row into an output", "two outputs one row apart"),
                                    f"{G}::test_key_switch_batch_aliasing"),
    "hefx_rotate_multiply_plain_batch": _row(IN_PLACE, ("d_ct_out[i] == d_ct_in[i]",),
                                             ("d_ct_out[1] == d_ct_in[0]", "an output on a plaintext", "two outputs one row apart"),
                                             f"{G}::test_key_switch_batch_aliasing"),
    "hefx_apply_galois_add_batch": _row(IN_PLACE, ("d_acc_out[i] == d_acc_in[i]", "d_ct_out[i] == d_ct_in[i]"),
                                        ("a sum on the other item's sum, on a rotation output or on an input",
                                         "d_acc_in[i] one row into d_acc_out[i]", "d_acc_in[0] == d_acc_out[1]"),
                                        f"{G}::test_apply_galois_add_batch_aliasing"),
    "hefx_rotate_add_chain": _row(IN_PLACE, ("d_ct_out[i] == d_ct_in[i]",), ("any two of the 2n outputs overlapping",),
                                  f"{G}::test_rotate_add_chain_aliasing"),
    "hefx_apply_galois_forest": _row(NO_OVERLAP, (), ("outputs on one another", "an output on an external input", "an output on a plaintext"),
                                     f"{G}::test_apply_galois_forest_refusals"),
    "hefx_linear_transform_cipher": _row(NO_OVERLAP, (), ("d_out3 on d_ct", "d_out3 on a diagonal", "a diagonal one row into d_out3"),
                                         f"{G}::test_linear_transform_cipher_refusals"),
    "hefx_multiply_sum": _row(NO_OVERLAP, (), ("an output on an input of the other group", "two outputs one row apart"),
                              f"{G}::test_multiply_sum_refusals"),
}

# hefx_add_many with d_out == d_in[i]: (n, i) on both sides of every path of add_many_impl -- one launch (n <= 48), two
# launches (49..96: the form that read a partial sum before the fix), the table level (97..)
ADD_MANY_IN_PLACE = [(3, 0), (3, 2), (48, 47), (49, 48), (60, 59), (60, 3), (96, 95), (97, 96), (150, 149)]
# n = 60 from a pool of four buffers, out the one that sits at these positions (a repeated input as the output)
ADD_MANY_POOL_N, ADD_MANY_POOL_OUT_AT = 60, (1, 50, 59)
