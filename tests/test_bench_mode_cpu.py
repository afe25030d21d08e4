"""bench.py's launch-mode selection (CPU only): a plain `python bench.py
--gpus N` with N > 1 and no launcher runs in-process over devices 0..N-1
(the driver's bench command must not exit without a line);
under torch.distributed.run each rank renders its rows."""
import importlib.util
import os

import pytest

from conftest import ROOT


@pytest.fixture(scope="module")
def bench():
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(ROOT, "bench.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_mode_selection(bench):
    assert bench.select_mode(1, 1, False) == "single"
    for n in (2, 4, 8):
        assert bench.select_mode(1, n, False) == "in-process"  # no launcher: never an exit
        assert bench.select_mode(n, n, False) == "ranks"
    assert bench.select_mode(1, 1, True) == "in-process"
    with pytest.raises(ValueError):
        bench.select_mode(4, 8, False)  # launcher and --gpus disagree
    with pytest.raises(ValueError):
        bench.select_mode(2, 2, True)


def test_device_list(bench):
    assert bench.parse_devices(None, 8, 8) == list(range(8))
    assert bench.parse_devices("0,0,0,0,0,0,0,0", 8, 1) == [0] * 8
    with pytest.raises(ValueError):
        bench.parse_devices(None, 8, 1)  # eight GPUs asked, one present: an error, not a silent 1-GPU line
    with pytest.raises(ValueError):
        bench.parse_devices("0,1", 3, 4)
    with pytest.raises(ValueError):
        bench.parse_devices("0,5", 2, 4)


def test_dump_rows_sample(bench):
    """--dump-outputs keeps a whole frame that fits in 64 MB and a fixed,
    seeded, ascending row sample of a larger one (C5: 3840 x 2160 x 3 f32)."""
    assert bench.dump_rows(1080, 1920 * 3 * 4) is None  # C2: 24.9 MB
    row = 3840 * 3 * 4
    rows = bench.dump_rows(2160, row)
    assert len(rows) == 64 * 1000 * 1000 // row and len(rows) * row <= 64 * 1000 * 1000
    assert len(set(rows.tolist())) == len(rows) and rows.min() >= 0 and rows.max() < 2160
    assert (rows[1:] > rows[:-1]).all()
    assert (bench.dump_rows(2160, row) == rows).all()  # the same rows every run
    assert bench.dump_rows(10, 100, max_bytes=250).tolist() == bench.dump_rows(10, 100, max_bytes=299).tolist()
    assert len(bench.dump_rows(10, 100, max_bytes=50)) == 1  # never empty


def test_dump_outputs_file(bench, tmp_path):
    import numpy as np
    import torch
    frame = torch.arange(5 * 7 * 3, dtype=torch.float32).reshape(5, 7, 3)
    d = tmp_path / "new" / "dir"
    bench.dump_outputs(str(d), frame)
    assert sorted(os.listdir(d)) == ["frame.npy"]
    a = np.load(d / "frame.npy")
    assert a.dtype == np.float32 and a.shape == (5, 7, 3)
    assert (a == frame.numpy()).all()


def test_gather_mode_names_match_header(bench):
    text = open(os.path.join(ROOT, "include", "rt_mi355x.h")).read()
    for code, name in ((0, "NONE"), (1, "RCCL_COMM"), (2, "RCCL_DEVICES"), (3, "PEER_COPY")):
        assert f"#define RT_GATHER_{name} {code}" in text
    assert set(bench.GATHER_MODES) == {0, 1, 2, 3}
