"""CPU: bench.py's HOST logic end to end — argument handling, the timed bracket, the roofline / counters / traffic bookkeeping,
the guard around the one-hashgraph split and the ONE JSON line of the driver's contract — with the CPU oracle standing in for
the device (tests/oracle_backend.py) at a toy size.  Nothing here measures anything: it only keeps a mistake in the bench
script (an unbound name, a missing key) from costing the round's measurement."""
import importlib
import json
import sys

import numpy as np
import pytest

import oracle_backend


class BenchStandIn(oracle_backend.OracleHashgraph):
    """OracleHashgraph + the measurement entry points bench.py uses (rewind / reset / profiling / timings / counters)."""

    def __init__(self, n_members, stake=None, coin_period=6, device=0):
        super().__init__(n_members, stake, coin_period, device)
        self._args = (n_members, stake, coin_period)
        self._stream = []
        self._base = {}

    def reserve(self, n_events):
        pass

    def append_events(self, creator, self_parent, other_parent, t=None, sig=None):
        self._stream.append((creator, self_parent, other_parent, t, sig))
        super().append_events(creator, self_parent, other_parent, t, sig)

    def _fresh(self, keep_events):
        L = importlib.import_module("py-swirld_amd._lib")
        done = self.counters()
        self._base = {k: done.get(k, 0) for k, _ in L.Counters._fields_}   # counters are cumulative over rewinds
        stream = self._stream if keep_events else []
        self.__dict__.pop("_head", None)
        oracle_backend.OracleHashgraph.__init__(self, *self._args)
        self._stream = []
        for part in stream:
            self.append_events(*part)

    def rewind(self):
        self._fresh(True)

    def reset(self):
        self._fresh(False)

    def synchronize(self):
        pass

    def set_profiling(self, enable=True):
        pass

    def timings(self):
        L = importlib.import_module("py-swirld_amd._lib")
        return {k: (1 if k.endswith("_launches") else 1.0) for k, _ in L.Timings._fields_}

    def counters(self):
        L = importlib.import_module("py-swirld_amd._lib")
        c = super().counters()
        return {k: int(c.get(k, 0)) + int(self._base.get(k, 0)) for k, _ in L.Counters._fields_}

    tally_kernel = "k_tally_bits"


def test_bench_prints_the_contract_line(pkg, monkeypatch, capsys):
    import torch
    bench = importlib.import_module("bench")
    monkeypatch.setattr(pkg, "Hashgraph", BenchStandIn)
    monkeypatch.setattr(torch.cuda, "is_available", lambda: True)
    monkeypatch.setattr(torch.cuda, "set_device", lambda *a, **k: None)
    monkeypatch.setattr(torch.cuda, "synchronize", lambda *a, **k: None)
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--members", "16", "--events", "6000", "--steps", "2", "--warmup", "1",
                                      "--contexts", "2", "--concurrent", "2", "--cpu-sample", "3000", "--e2e-steps", "1",
                                      "--reference-events", "0", "--full"])
    bench.main()
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("{")]
    assert len(lines) == 1                                    # ONE JSON line
    d = json.loads(lines[0])
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
              "vs_baseline", "dtype", "data", "config", "roofline", "cpu_baseline"):
        assert k in d, k
    assert d["n_gpus"] == 1 and d["steps"] == 2 and d["warmup"] == 1 and d["higher_is_better"] is True
    assert d["unit"] == "events/s" and d["scaling"] == "weak" and d["vs_baseline"] is None and d["data"] == "synthetic"
    assert d["value"] > 0 and abs(d["value"] - 6000 / (d["ms_per_step"] * 1e-3)) / d["value"] < 0.01
    assert "workload" in d["config"] and "timed_region" in d["config"] and "model" not in d["config"]
    r = d["roofline"]
    for k in ("bound", "achieved", "peak", "unit", "frac", "traffic", "kernels", "path_frac", "hbm_bytes_per_step_pmc", "traffic_stale"):
        assert k in r, k
    assert r["traffic_stale"] is False                       # (profiles/traffic.json belongs to this tree's kernel source)
    assert r["frac"] == r["path_frac"] and r["bound"] == "hbm"   # the headline fraction is the whole path's
    assert r["traffic"] is None and "none" in r["traffic_source"]   # (no counter pass exists for a 16-member workload: nothing is quoted)
    assert r["dominant_kernel"]["served_by"].startswith("hbm")    # an L2-served family is never the kernel named under bound "hbm"
    assert {"k_resolve_band", "k_tally_bits", "k_elections"} <= {k["kernel"] for k in r["kernels"]}
    c = d["cpu_baseline"]
    assert c["kind"] == "port" and c["cores"] == 1 and c["value"] > 0 and "sample" in c
    assert d["strong"] is None and d["value_strong"] is None
    assert d["value_end_to_end"] > 0 and d["find_order_ms"] >= 0 and d["value_concurrent_contexts"]["contexts"] == 2
    assert d["roofline"]["counters"]["round_iterations"] >= 0 and "finalize_from_rows" in d["roofline"]["counters"]


def _plain_run(pkg, monkeypatch, capsys, extra):
    import torch
    bench = importlib.import_module("bench")
    monkeypatch.setattr(pkg, "Hashgraph", BenchStandIn)
    monkeypatch.setattr(torch.cuda, "is_available", lambda: True)
    monkeypatch.setattr(torch.cuda, "set_device", lambda *a, **k: None)
    monkeypatch.setattr(torch.cuda, "synchronize", lambda *a, **k: None)
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--members", "16", "--events", "6000", "--steps", "3", "--warmup", "1",
                                      "--contexts", "2"] + extra)
    bench.main()
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    return json.loads(lines[0])


def test_plain_run_times_only_the_steps(pkg, monkeypatch, capsys):
    """Without --full the line carries the headline fields; every figure that takes runs of its own is null."""
    calls = {"oracle": 0}
    from oracle import oracle as oracle_mod
    real = oracle_mod.Oracle

    class Counting(real):
        def __init__(self, *a, **k):
            calls["oracle"] += 1
            super().__init__(*a, **k)
    monkeypatch.setattr(oracle_mod, "Oracle", Counting)
    d = _plain_run(pkg, monkeypatch, capsys, [])
    assert d["metric"] == "events/sec through divide_rounds+decide_fame" and d["unit"] == "events/s"
    assert d["higher_is_better"] is True and d["dtype"] == "int32" and d["steps"] == 3 and d["warmup"] == 1
    assert d["value"] > 0 and abs(d["value"] - 6000 / (d["ms_per_step"] * 1e-3)) / d["value"] < 0.01
    for k in ("roofline", "cpu_baseline", "end_to_end", "value_end_to_end", "value_concurrent_contexts", "strong",
              "value_strong", "value_with_order", "find_order_ms"):
        assert d[k] is None, k
    assert calls["oracle"] == 0                              # no CPU baseline in a plain run


def test_steps_sets_the_number_of_timed_steps(pkg, monkeypatch, capsys):
    n_steps = {"n": 0}
    real = BenchStandIn.decide_fame

    def counting(self):
        n_steps["n"] += 1
        return real(self)
    monkeypatch.setattr(BenchStandIn, "decide_fame", counting)
    d = _plain_run(pkg, monkeypatch, capsys, ["--steps", "4", "--warmup", "2"])
    # one set-up pass per resident context (2), the warm-up steps, the timed steps: nothing else
    assert d["steps"] == 4 and n_steps["n"] == 2 + 2 + 4


def test_dump_outputs_are_the_last_steps_results(pkg, monkeypatch, capsys, tmp_path):
    from oracle.oracle import Oracle
    d = _plain_run(pkg, monkeypatch, capsys, ["--dump-outputs", str(tmp_path / "a")])
    _plain_run(pkg, monkeypatch, capsys, ["--dump-outputs", str(tmp_path / "b")])
    names = sorted(p.name for p in (tmp_path / "a").iterdir())
    assert names == ["can_see.npy", "famous.npy", "new_c.npy", "rounds.npy", "witnesses.npy"]
    total = 0
    for name in names:
        a, b = np.load(tmp_path / "a" / name), np.load(tmp_path / "b" / name)
        assert a.dtype in (np.float32, np.float64) and np.array_equal(a, b), name   # same arguments, same outputs
        total += a.nbytes
    assert total <= 64 << 20
    stream = pkg.synth_hashgraph(16, 6000, 3)
    o = Oracle(16)
    o.append_events(*stream)
    o.divide_rounds(0, 6000)
    new_c = o.decide_fame()
    out = {name[:-4]: np.load(tmp_path / "a" / name) for name in names}
    assert np.array_equal(out["rounds"], o.round) and np.array_equal(out["can_see"], o.can_see)
    assert np.array_equal(out["witnesses"], o.witnesses()) and list(out["new_c"]) == list(new_c)
    assert len(out["new_c"]) == d["config"]["new_c_last_step"]


def test_dump_outputs_samples_tables_beyond_the_cap(tmp_path, monkeypatch):
    """A table larger than its share of the 64 MB is written as a fixed, seeded sample of rows, with the row indices."""
    bench = importlib.import_module("bench")
    monkeypatch.setattr(bench, "DUMP_CAP_BYTES", 4 << 20)

    class Big:
        n, num_events = 64, 40000
        cs = np.arange(40000 * 64, dtype=np.int32).reshape(40000, 64)

        def rounds(self):
            return np.arange(self.num_events, dtype=np.int32) // 100

        def witnesses(self):
            return np.zeros((400, self.n), np.int32)

        def famous(self):
            return np.ones((400, self.n), np.int8)

        def can_see(self, first=0, K=None):
            return self.cs[first:first + (self.num_events - first if K is None else K)]

    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), Big(), [1, 2], seed=3)
    rows = np.load(tmp_path / "a" / "can_see_rows.npy").astype(np.int64)
    cs = np.load(tmp_path / "a" / "can_see.npy")
    assert cs.nbytes <= (4 << 20) // 4 and len(rows) == len(cs) and np.all(np.diff(rows) > 0)
    assert np.array_equal(cs, Big.cs[rows])
    assert np.array_equal(rows, np.load(tmp_path / "b" / "can_see_rows.npy").astype(np.int64))
    assert np.load(tmp_path / "a" / "rounds.npy").shape == (40000,)          # within its share: whole
