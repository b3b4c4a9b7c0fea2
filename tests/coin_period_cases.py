"""The fixtures of tests/golden/coin_period/ (the unmodified reference run at a coin period other than 6; generator:
tests/golden/make_coin_period_golden.py), for tests/test_coin_period_host.py and tests/test_gpu_coin_period.py."""
import glob
import os
import re

from conftest import GOLDEN_DIR, load_golden  # noqa: F401

SUB = "coin_period"
FORKED = ("n8_s11_forks", "n8_s12_forks_chunk9", "n5_s13_forks_chunk1", "n12_s14_forks_stake_chunk40")
# a fixture that cannot hold a coin vote: no member's stake lets a round complete, so there is one round and no election
NO_ELECTION = ("n6_s3_stuck_stake_c2", "n6_s3_stuck_stake_c3")


def names():
    return sorted(os.path.splitext(os.path.basename(p))[0] for p in glob.glob(os.path.join(GOLDEN_DIR, SUB, "*.npz")))


def period_of(name):
    return int(re.search(r"_c(\d+)$", name).group(1))


def stream_of(name):
    return re.sub(r"_c\d+$", "", name)


def is_forked(name):
    return stream_of(name) in FORKED


def load(name):
    g = load_golden(os.path.join(SUB, name))
    g["coin_period"] = int(g["coin_period"])
    assert g["coin_period"] == period_of(name)
    for k in ("coin_votes", "coin_flips", "max_vote_distance"):
        g[k] = int(g[k])
    return g


def new_c_of(g, call):
    return list(g["new_c_flat"][g["new_c_off"][call]:g["new_c_off"][call + 1]])


def tx_of(g, call):
    return list(g["transactions"][g["tx_off"][call]:g["tx_off"][call + 1]])
