"""The CPU oracle's elementwise proxes on directed operands -- branch thresholds of the 14 Function1D maps, one ulp either side of
them, signed zeros, subnormals, squares that underflow or overflow, the largest finite numbers, infinities, NaN (tests/elem_edge_cases.py)
-- against the answers of the reference's own functors, stored in tests/golden/elementwise_edges.npz by tests/golden/make_golden.py
(edges): one digest per case (bit for bit up to the sign of zero and the NaN payload), the Function1DLq answers as values compared
with close_lq.  Where oracle/_ref is built the reference's live answers must match the same record.  No GPU.
"""
import functools
import os

import numpy as np
import pytest

import elem_edge_cases as E
import oracle
from oracle import ref
from test_oracle_pinning import DTYPES, GOLD, answer_digest, close_lq

# per data type: 13 functions x 4 families x 2 invert flags, and lq with its four alphas in the exact family; x 13 shapes
CASES_PER_DTYPE = (13 * 8 + (4 + 3) * 2) * len(E.RECORD_SHAPES)


@functools.lru_cache(maxsize=None)
def _record():
    g = dict(np.load(os.path.join(GOLD, "elementwise_edges.npz")))
    keys, dig = g.pop("digest_keys"), g.pop("digests")
    g.update((k.decode(), bytes(d).hex()) for k, d in zip(keys, dig))
    return g


def test_the_generator_is_the_one_the_oracle_knows():
    assert E.FUNCTIONS == tuple(oracle.FUNCTIONS)
    assert len(E.RECORD_SHAPES) == 13


def test_thresholds_are_hit_exactly():
    """the boundary operand of every function makes its branch condition an equality (asserted in rational arithmetic by
    exact_params) and is among the operands, next to its two neighbours, a NaN and an overflowing value in the first wave"""
    for dt in DTYPES:
        for fn in E.FUNCTIONS:
            for step in (0.5, 2.0):
                alpha, beta, x0 = E.exact_params(fn, step)
                v = E.operand_values(dt, step, alpha, beta, x0)
                assert len(v) <= 64 and np.isnan(v).sum() == 1 and np.isinf(v).sum() == 2
                for w in (x0, np.nextafter(dt(x0), dt(np.inf)), np.nextafter(dt(x0), dt(-np.inf)), -x0):
                    assert (v == dt(w)).any(), (fn, step, w)
                with np.errstate(over="ignore"):
                    assert np.isinf(v[np.isfinite(v)] ** 2).any() and ((v != 0) & (v * v == 0)).any()


@pytest.mark.parametrize("dtype", DTYPES)
def test_oracle_equals_the_reference_on_the_directed_operands(dtype):
    rec = _record()
    checked = 0
    for name, args in E.cases(dtype):
        exp = rec[name]
        for who, a in [("oracle", oracle.prox_elem(*args))] + ([("live reference", ref.prox_elem(*args))] if ref.available() else []):
            if args[1] == "lq":
                assert close_lq(a, exp, dtype), (who, name)
            else:
                assert answer_digest(a) == exp, (who, name)
        checked += 1
    assert checked == CASES_PER_DTYPE
    assert len(rec) == 2 * CASES_PER_DTYPE
