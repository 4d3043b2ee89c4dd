"""bench.py's plain / --full split and --dump-outputs.

A plain run measures the headline alone; --full adds the sub-results and the CPU legs.
--dump-outputs writes what the last timed step computed, float32 / float64, large arrays
as a fixed sample, under 64 MB in all."""
import os

import numpy as np
import pytest

DUMP_LIMIT_BYTES = 64 * 10 ** 6


def test_plain_run_is_the_default():
    import bench
    a = bench.parse(["--gpus", "1", "--steps", "7", "--warmup", "2"])
    assert not a.full and a.dump_outputs is None
    assert (a.steps, a.warmup) == (7, 2)
    b = bench.parse(["--full", "--dump-outputs", "somewhere"])
    assert b.full and b.dump_outputs == "somewhere"


def test_dump_outputs_dtypes_and_fixed_sample(tmp_path):
    import bench
    cap = bench.DUMP_MAX_VALUES
    assert 4 * cap * 4 < DUMP_LIMIT_BYTES          # the train step's four large arrays
    big = (np.arange(cap + 1000) % 2048).astype(np.float16).reshape(-1, 8)
    arrays = {"small": np.arange(12, dtype=np.float16).reshape(3, 4), "stats": np.array([1.5, -2.0]),
              "big": big}
    d1, d2 = str(tmp_path / "a"), str(tmp_path / "b")
    bench.dump_outputs(d1, arrays)
    bench.dump_outputs(d2, arrays)
    assert sorted(os.listdir(d1)) == ["big.npy", "small.npy", "stats.npy"]
    small, stats, got = (np.load(os.path.join(d1, n + ".npy")) for n in ("small", "stats", "big"))
    assert small.dtype == np.float32 and np.array_equal(small, arrays["small"])
    assert stats.dtype == np.float64 and np.array_equal(stats, arrays["stats"])
    # the sample: cap values of the flattened array at seeded, ascending positions
    assert got.dtype == np.float32 and got.shape == (cap,)
    idx = np.sort(np.random.default_rng(1234).integers(0, big.size, cap))
    assert np.array_equal(got, big.reshape(-1)[idx])
    assert np.array_equal(got, np.load(os.path.join(d2, "big.npy")))


@pytest.mark.gpu
def test_dump_outputs_of_the_last_timed_step(gpu, tmp_path):
    """the train step at 2 egs: every array a caller of the step holds is written, finite,
    and of the step (the objective's statistics cover both egs; the gradients are not zero)"""
    import bench
    a = bench.parse(["--egs", "2"])
    head, _ = bench.run_workload(a, a.xconfig, "train", False, 0, 1, None, 2, 1, True, dump=str(tmp_path))
    assert head["steps"] == 2 and len(head["step_ms"]) == 2
    names = ["grads", "objective", "output", "output_grad", "params"]
    assert sorted(os.listdir(tmp_path)) == [n + ".npy" for n in names]
    arr = {n: np.load(tmp_path / (n + ".npy")) for n in names}
    assert sum(v.nbytes for v in arr.values()) < DUMP_LIMIT_BYTES
    for n, v in arr.items():
        assert v.dtype == (np.float64 if n == "objective" else np.float32), n
        assert np.isfinite(v).all(), n
    assert np.array_equal(arr["objective"], np.asarray(head["stats"], np.float64))
    assert arr["objective"][4] == a.egs
    cap = bench.DUMP_MAX_VALUES
    whole = (head["obj_rows"], 3080)                             # whole up to the cap, else the sample
    assert arr["output"].shape == (whole if whole[0] * whole[1] <= cap else (cap,))
    assert arr["output_grad"].shape == arr["output"].shape
    assert arr["params"].shape == (cap,)
    for n in ("output", "output_grad", "grads", "params"):
        assert np.count_nonzero(arr[n]) > arr[n].size // 2, n
    assert gpu.core.kf_peek_error() == 0
