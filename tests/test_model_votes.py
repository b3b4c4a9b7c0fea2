"""CPU: tests/model_votes.py, the specification of the votes table of sw_export_votes, against the reference's complete
`votes` dict in every fork-free golden — batch and incremental call schedules, stakes, coin rounds."""
import numpy as np
import pytest

import model_votes as mv
from conftest import golden_names, load_golden

FORKFREE = [n for n in golden_names() if "forks" not in n]
_STATS = {}


def as_set(tr):
    return {(int(y), int(x), int(v)) for y, x, v in tr}


@pytest.mark.parametrize("name", FORKFREE)
def test_model_equals_the_reference_votes(name):
    g = load_golden(name)
    t = mv.model_votes(g)
    tr = mv.triples(t["row_voter"], t["row_cand_round"], t["exists"], t["value"], g["witnesses"])
    exp = as_set(g["votes"])
    assert len(exp) == len(g["votes"])
    assert len(tr) == len(exp) == t["n_entries"], "same size"
    assert as_set(tr) == exp, "no extras, nothing missing"
    assert not (t["value"] & ~t["exists"]).any()
    rnd = g["round"]
    keys = list(zip(rnd[t["row_voter"]].tolist(), t["row_voter"].tolist(), t["row_cand_round"].tolist()))
    assert keys == sorted(keys) and len(set(keys)) == len(keys)
    if name == "n6_s3_stuck_stake":
        assert len(t["row_voter"]) == 0, "no member's stake lets a round complete: no election, no votes"
    _STATS[name] = (t["n_coin"], t["n_weighted"])


def test_the_fixtures_cover_what_the_table_depends_on():
    dist = {}
    for name in FORKFREE:
        g = load_golden(name)
        v = g["votes"]
        if name != "n6_s3_stuck_stake":
            assert len(v) > 0, name
        dist[name] = int((g["round"][v[:, 0]] - g["round"][v[:, 1]]).max()) if len(v) else 0
    far = [k for k, d in dist.items() if d >= mv.COIN_PERIOD]
    assert any(k.startswith("n4_") for k in far) and "n10_s1_stake" in far and "n16_s8_slow" in far, dist
    for name in ("n10_s1_stake", "n12_s2_stake"):
        assert not (load_golden(name)["stake"] == 1).all()
    assert any("_chunk" in k for k in FORKFREE) and "n4_mainloop_node0" in FORKFREE
    assert len(load_golden("n4_mainloop_node0")["batches"]) > 1


def test_coin_branch_and_weighted_majority_were_checked():
    """(after the parametrised test, whose runs it counts; computes what is missing when run alone)"""
    for name in ("n4_s1_batch", "n10_s1_stake"):
        if name not in _STATS:
            t = mv.model_votes(load_golden(name))
            _STATS[name] = (t["n_coin"], t["n_weighted"])
    assert sum(c for c, _ in _STATS.values()) > 0, "no checked entry took the coin branch (swirld.py:272)"
    assert sum(w for _, w in _STATS.values()) > 0, "no checked entry has a stake-weighted majority"
