"""bench.py: the driver's contract (one JSON line, the keys and types it reads) and the synthetic
scalar generator."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def test_gen_scalars_are_canonical_and_deterministic():
    import bench
    for name in ("bn254_g1", "grumpkin"):
        m = bench.ORDER[name]
        a = bench.gen_scalars(5000, m, 42); b = bench.gen_scalars(5000, m, 42); c = bench.gen_scalars(5000, m, 43)
        assert a.shape == (5000, 32) and a.dtype == np.uint8
        assert np.array_equal(a, b) and not np.array_equal(a, c)
        vals = [int.from_bytes(r.tobytes(), "little") for r in a]
        assert max(vals) < m and len(set(vals)) > 4990
        assert max(vals) > m >> 3          # spread over the whole range, not a narrow band


@pytest.mark.gpu
@pytest.mark.parametrize("extra", [[], ["--workload", "lhs"]], ids=["msm", "lhs"])
def test_bench_prints_one_contract_line(extra):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1", "--logn", "12",
           "--cpu-sample-log", "10"] + extra
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, r.stdout
    d = json.loads(lines[0])
    for k, t in (("metric", str), ("value", float), ("unit", str), ("n_gpus", int), ("steps", int), ("warmup", int),
                 ("ms_per_step", float), ("higher_is_better", bool), ("scaling", str), ("dtype", str), ("data", str), ("config", dict)):
        assert isinstance(d[k], t), (k, d[k])
    assert d["vs_baseline"] is None and d["n_gpus"] == 1 and d["steps"] == 2 and d["warmup"] == 1 and d["higher_is_better"] is True
    assert d["value"] > 0 and "workload" in d["config"] and d["config"]["bit_exact"] is True
    ro = d["roofline"]
    assert ro["bound"] in ("hbm", "mfma") and ro["unit"] == "GB/s" and ro["peak"] == 8000.0
    assert abs(ro["frac"] - ro["achieved"] / ro["peak"]) < 1e-5 and ro["kernel"] == "k_accum1" and ro["kernel_ms"] > 0
    vi = ro["valu_issue"]
    assert 0 < vi["frac"] <= 1.0 and vi["peak_clock_ghz"] == 2.4          # priced at the guide's maximum clock: <= 1 by construction
    assert vi["clock_ghz_measured"] is None or 0.5 < vi["clock_ghz_measured"] <= 2.5
    assert "timed result vs walk identity" in d["config"]["bit_exact_checks"] and "sample vs oracle" in d["config"]["bit_exact_checks"]
    cb = d["cpu_baseline"]
    assert cb["kind"] in ("port", "reference") and cb["value"] > 0 and cb["cores"] >= 1 and isinstance(cb["sample"], str)
    # the CPU leg follows the workload: the lhs line times the serial compute_lhs_witness restatement, not best_multiexp
    assert ("compute_lhs_witness" in cb["sample"]) == (extra != [])
    if extra:
        assert cb["cores"] == 1


@pytest.mark.gpu
def test_bench_lhs_witness_line():
    """--workload lhs_witness: compute_lhs_witness in full as a contract-shaped, self-verified line"""
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--workload", "lhs_witness", "--steps", "2", "--warmup", "1", "--logn", "10",
           "--cpu-sample-log", "7"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, r.stdout
    d = json.loads(lines[0])
    assert d["unit"] == "pairs/s" and d["value"] > 0 and d["n_gpus"] == 1 and d["steps"] == 2 and d["vs_baseline"] is None
    assert d["config"]["bit_exact"] is True and "timed carry vs walk identity" in d["config"]["bit_exact_checks"]
    assert any("every coefficient" in c for c in d["config"]["bit_exact_checks"])
    ro = d["roofline"]
    assert ro["bound"] == "hbm" and ro["unit"] == "GB/s" and ro["peak"] == 8000.0 and ro["traffic"] is None
    assert abs(ro["frac"] - ro["achieved"] / ro["peak"]) < 1e-3 and "k_ntt_tile" in ro["kernel"] and ro["kernel_ms"] > 0
    assert 0 < ro["valu_butterflies"]["frac"] <= 1.0
    assert set(ro["phases_ms"]) == {"msm_core", "point_lists", "merge_forest", "coefficient_copy"}
    cb = d["cpu_baseline"]
    assert cb["kind"] == "port" and cb["cores"] >= 1 and cb["value"] > 0 and "compute_lhs_witness" in cb["sample"]


def test_dump_outputs_writes_exact_float_words(tmp_path):
    """--dump-outputs: Jacobian points are written as their canonical affine x || y, 32-bit words in float64 (exact)"""
    import bench
    from oracle import cref
    g = cref.generator(0)
    jac = np.stack([cref.scalar_mul(0, k, g) for k in (1, 2, 3)])
    idx = np.array([[0, 3, 3, 1]], np.uintp)
    bench.dump_outputs(str(tmp_path), 0, {"pts": jac, "one": jac[1]}, {"index": idx})
    assert sorted(os.listdir(tmp_path)) == ["index.npy", "one.npy", "pts.npy"]
    aff = np.load(tmp_path / "pts.npy")
    assert aff.dtype == np.float64 and aff.shape == (3, 16)
    for i in range(3):
        assert aff[i].astype(np.uint32).tobytes() == cref.jac_to_canonical(0, jac[i])
    assert np.array_equal(np.load(tmp_path / "one.npy"), aff[1])
    # another Jacobian representative of the same points, (l^2 X, l^3 Y, l Z), gives the same file
    from oracle import pyref
    c, lm = pyref.BN254_G1, pyref.BN254_G1.to_mont(7)
    limb = lambda v: np.frombuffer(v.to_bytes(32, "little"), np.uint64)
    two = jac.copy()
    for i in range(3):
        x, y, z = (int.from_bytes(jac[i, 4 * k:4 * k + 4].tobytes(), "little") for k in range(3))
        l2 = c.montmul(lm, lm)
        two[i, 0:4], two[i, 4:8], two[i, 8:12] = limb(c.montmul(x, l2)), limb(c.montmul(y, c.montmul(l2, lm))), limb(c.montmul(z, lm))
    assert not np.array_equal(two, jac)
    bench.dump_outputs(str(tmp_path / "again"), 0, {"pts": two})
    assert np.array_equal(np.load(tmp_path / "again" / "pts.npy"), aff)
    assert np.array_equal(np.load(tmp_path / "index.npy"), idx.astype(np.float64))


def test_dump_coefficient_sample_is_seeded_and_indexed(monkeypatch):
    """the witness coefficients are sampled with a fixed seed over all functions in index order"""
    import bench
    mem = np.arange(4 * 300, dtype=np.uint64).reshape(300, 4) * np.uint64(0x100000001)
    monkeypatch.setattr(bench, "_download_elems", lambda ctx, buf, off, count: mem[off:off + count].copy())
    index = np.array([[0, 10, 100, 0], [20, 5, 200, 50]], np.uintp)
    a = bench.sample_coefficients(None, None, index)
    b = bench.sample_coefficients(None, None, index)
    ks = a["lhs_witness_coeff_sample_k"].astype(np.int64)
    assert np.array_equal(ks, b["lhs_witness_coeff_sample_k"].astype(np.int64)) and ks.size == 65
    flat = np.concatenate([mem[0:10], mem[20:25], mem[200:250]])          # the 65 coefficients in numbering order
    assert np.array_equal(a["lhs_witness_coeff_sample"].astype(np.uint32).view(np.uint64), flat[ks])
    big = np.arange(4 * 200000, dtype=np.uint64).reshape(200000, 4)
    monkeypatch.setattr(bench, "_download_elems", lambda ctx, buf, off, count: big[off:off + count].copy())
    index = np.array([[0, 90000, 90000, 0], [100000, 60000, 160000, 40000]], np.uintp)
    c = bench.sample_coefficients(None, None, index)
    ks = c["lhs_witness_coeff_sample_k"].astype(np.int64)
    assert ks.size == bench.DUMP_COEFF_SAMPLE == np.unique(ks).size and ks.max() < 190000
    assert np.array_equal(ks, bench.sample_coefficients(None, None, index)["lhs_witness_coeff_sample_k"].astype(np.int64))
    flat = np.concatenate([big[0:90000], big[100000:160000], big[160000:200000]])
    assert np.array_equal(c["lhs_witness_coeff_sample"].astype(np.uint32).view(np.uint64), flat[ks])


@pytest.mark.gpu
@pytest.mark.parametrize("extra", [["--logn", "12"], ["--workload", "lhs", "--logn", "12"], ["--workload", "lhs_witness", "--logn", "10"]],
                         ids=["msm", "lhs", "lhs_witness"])
def test_bench_dump_outputs_are_reproducible(tmp_path, extra):
    """two runs with the same arguments dump the same float arrays, within the 64 MB bound"""
    dumps = []
    for run in ("a", "b"):
        cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--no-cpu-baseline",
               "--dump-outputs", str(tmp_path / run)] + extra
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT)
        assert r.returncode == 0, r.stderr[-2000:]
        d = json.loads([ln for ln in r.stdout.splitlines() if ln.strip()][-1])
        assert d["steps"] == 3 and d["ms_per_step"] > 0 and d["config"]["bit_exact"] is True
        files = sorted(os.listdir(tmp_path / run))
        assert files and all(f.endswith(".npy") for f in files)
        dumps.append({f: np.load(tmp_path / run / f) for f in files})
    assert dumps[0].keys() == dumps[1].keys()
    assert sum(a.nbytes for a in dumps[0].values()) <= 64 << 20
    for f, a in dumps[0].items():
        assert a.dtype in (np.float32, np.float64) and a.size > 0, f
        assert np.array_equal(a, dumps[1][f]), f
