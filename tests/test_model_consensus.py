"""CPU: tests/model_consensus.py (SURVEY.md Appendix A, Q10-Q12 in numpy) against the reference's own round received and
consensus timestamps (tests/golden/consensus, captured by tests/golden/make_consensus_golden.py): every fixture, both
variants, every ordered event — integer and timestamp bit for bit; events the reference did not order come out as not
ordered.  The inputs (can_see rows, witness and fame tables, parents, heights, stake, the rounds of every call) are the
stored goldens'."""
import os
import re

import numpy as np
import pytest

import model_consensus as mc
from conftest import GOLDEN_DIR, load_golden

CONS_DIR = os.path.join(GOLDEN_DIR, "consensus")
NAMES = sorted(os.path.splitext(f)[0] for f in os.listdir(CONS_DIR) if f.endswith(".npz"))
VARIANTS = ("asis", "wallclock")


def load_consensus(name):
    with np.load(os.path.join(CONS_DIR, name + ".npz")) as z:
        return {k: z[k] for k in z.files}


def variant(g, f, v):
    """(t, transactions, tx_off, round_received, consensus_time) of one variant."""
    if v == "asis":
        return g["t"], g["transactions"], g["tx_off"], f["asis_round_received"], f["asis_consensus_time"]
    return f["wallclock_t"], f["wallclock_transactions"], f["wallclock_tx_off"], f["wallclock_round_received"], f["wallclock_consensus_time"]


def same_bits(a, b):
    return np.array_equal(np.asarray(a, np.float64).view(np.uint64), np.asarray(b, np.float64).view(np.uint64))


def test_fixture_set_is_every_fork_free_case():
    src = open(os.path.join(GOLDEN_DIR, "make_golden.py")).read()
    block = src[src.index("CASES = ["):]
    block = block[:block.index("\n]")]
    cases = re.findall(r'^\s*\("([A-Za-z0-9_]+)",', block, re.M)
    assert len(cases) == 21 and not any("forks" in c for c in cases) and NAMES == sorted(cases)


@pytest.mark.parametrize("v", VARIANTS)
@pytest.mark.parametrize("name", NAMES)
def test_model_equals_the_reference(name, v):
    g, f = load_golden(name), load_consensus(name)
    t, tx, tx_off, rr, cts = variant(g, f, v)
    N = len(g["creator"])
    ordered = np.zeros(N, bool)
    ordered[tx] = True
    # the fixture itself: -1 / NaN exactly on the events that are not ordered, the schedule's call boundaries
    assert np.array_equal(rr >= 0, ordered) and np.array_equal(~np.isnan(cts), ordered)
    assert len(tx_off) == len(g["batches"]) + 1 and tx_off[-1] == len(tx)
    fam = mc.famous_table(g["witnesses"], g["famous"])
    got_rr, got_cts = mc.consensus_values(np.arange(N), g["new_c_flat"], g["can_see"], g["witnesses"], fam, g["creator"],
                                          g["self_parent"], g["height"], t, g["stake"])
    assert np.array_equal(got_rr, rr)
    assert same_bits(got_cts[ordered], cts[ordered]) and np.all(np.isnan(got_cts[~ordered]))
    # along each call's part of the order, (round received, consensus time) never decreases (swirld.py:306-309)
    for a, b in zip(tx_off[:-1], tx_off[1:]):
        assert mc.order_key_ok(tx[a:b], rr, cts)


def test_wallclock_variant_uses_the_whole_mantissa():
    """what the variant is for: with t = float(index) every consensus time is an integer or a half — a value carried through
    a float32, or rounded to a coarser grid, would still compare equal; the wall-clock times near 1.7e9 need the low bits of
    the double, and the sum of two of them rounds"""
    g, f = load_golden("n16_s3_batch"), load_consensus("n16_s3_batch")
    for v, expect in (("asis", False), ("wallclock", True)):
        t, tx, _, _, cts = variant(g, f, v)
        c = cts[tx]
        assert bool((c.astype(np.float32).astype(np.float64) != c).any()) == expect, v
        assert bool((np.round(c * 2) != c * 2).any()) == expect, v
