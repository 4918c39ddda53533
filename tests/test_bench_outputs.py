"""bench.py's plain run and ``--dump-outputs``: a plain run prints the headline line only (``--full`` holds every
figure that takes runs of its own), ``--steps`` sets the number of timed steps, and the dumped arrays are
float32 / float64, within ``bench.DUMP_BYTES`` in all and identical from run to run."""

from __future__ import annotations

import json
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import bench

HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")
FULL_ONLY = ("roofline", "network", "data_parallel", "cpu_baseline", "speedup_vs_cpu")


def test_full_and_dump_are_off_by_default() -> None:
    args = bench.parse(["--gpus", "1", "--steps", "7", "--warmup", "2"])
    assert args.full is False and args.dump_outputs is None and args.steps == 7
    args = bench.parse(["--full", "--dump-outputs", "out"])
    assert args.full is True and args.dump_outputs == "out"


def _fake_run(B: int, N: int):
    g = torch.Generator().manual_seed(5)
    slot = SimpleNamespace(contracts=torch.rand((B, 6), generator=g, dtype=torch.float64),
                           real_in=torch.rand((B, 6), generator=g),
                           targets=torch.complex(torch.rand((B, N), generator=g), torch.rand((B, N), generator=g)))
    other = SimpleNamespace(contracts=None, real_in=None, targets=None)
    session = SimpleNamespace(program=SimpleNamespace(slots=[other, slot, other, other], direct=True), steps=6)
    return session, slot, torch.nn.Linear(3, 2), SimpleNamespace(loss=1.5, grad_norm=0.25)


def test_dump_outputs_writes_the_last_steps_slot(tmp_path) -> None:
    session, slot, model, final = _fake_run(B=10, N=4)  # step 6 wrote slot (6 - 1) % 4 = 1
    shapes = bench.dump_outputs(str(tmp_path), session, model, final)
    got = {f[:-4]: np.load(tmp_path / f) for f in sorted(os.listdir(tmp_path))}
    assert sorted(got) == ["contracts", "loss_grad_norm", "network_input", "parameters", "targets"]
    assert {k: list(v.shape) for k, v in got.items()} == shapes
    assert all(v.dtype in (np.float32, np.float64) for v in got.values())
    assert np.array_equal(got["contracts"], slot.contracts.numpy())
    assert np.array_equal(got["network_input"], slot.real_in.numpy())
    assert np.array_equal(got["targets"][..., 0], slot.targets.real.numpy())
    assert np.array_equal(got["targets"][..., 1], slot.targets.imag.numpy())
    assert got["loss_grad_norm"].tolist() == [1.5, 0.25]
    assert np.array_equal(got["parameters"], np.concatenate([p.detach().numpy().ravel() for p in model.parameters()]))


def test_dump_outputs_cuts_to_a_fixed_row_sample_within_the_budget(tmp_path, monkeypatch) -> None:
    B, N = 300, 16
    session, slot, model, final = _fake_run(B, N)
    monkeypatch.setattr(bench, "DUMP_BYTES", 40000)  # the small arrays take 21,648 B; 143 target rows of 128 B fit
    bench.dump_outputs(str(tmp_path / "a"), session, model, final)
    bench.dump_outputs(str(tmp_path / "b"), session, model, final)
    total = 0
    for f in os.listdir(tmp_path / "a"):
        a, b = np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f)
        assert a.dtype == b.dtype and np.array_equal(a, b)
        total += a.nbytes
    assert total <= 40000
    small = 2 * 8 + 8 * 4 + B * 6 * 4 + B * 6 * 8
    rows = (40000 - small) // (N * 2 * 4)
    keep = np.sort(np.random.default_rng(0).choice(B, rows, replace=False))
    got = np.load(tmp_path / "a" / "targets.npy")
    assert 0 < rows < B and got.shape == (rows, N, 2)
    assert np.array_equal(got[..., 0], slot.targets.real.numpy()[keep])
    assert np.array_equal(np.load(tmp_path / "a" / "contracts.npy"), slot.contracts.numpy())  # whole: it fits


@pytest.mark.gpu
def test_plain_run_prints_the_headline_and_dumps_the_same_outputs_twice(tmp_path, monkeypatch, capsys) -> None:
    """Two plain runs of the e2e shape (4096 contracts x 512 paths) in this process: the line has the headline
    keys and none of --full's objects, --steps sets the timed steps, and both runs dump identical arrays."""
    lines = []
    for d in ("a", "b"):
        monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--config", "e2e", "--steps", "3", "--warmup", "2",
                                          "--dump-outputs", str(tmp_path / d)])
        bench.main()
        out = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("{")]
        assert len(out) == 1
        lines.append(json.loads(out[0]))
    B, _, N = bench.CONFIGS["e2e"][:3]
    for line in lines:
        assert all(k in line for k in HEADLINE) and not any(k in line for k in FULL_ONLY)
        assert line["steps"] == 3 and line["full"] is False and line["ms_per_step"] > 0
        assert line["value"] == pytest.approx(B * bench.CONFIGS["e2e"][2] * bench.CONFIGS["e2e"][3] * 3
                                              / (3 * line["ms_per_step"] * 1e-3))
        assert line["dumped_outputs"]["targets"] == [B, N, 2]
    total = 0
    for f in sorted(os.listdir(tmp_path / "a")):
        a, b = np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f)
        assert a.dtype in (np.float32, np.float64) and np.isfinite(a).all(), f
        assert np.array_equal(a, b), f
        total += a.nbytes
    assert sorted(os.listdir(tmp_path / "a")) == ["contracts.npy", "loss_grad_norm.npy", "network_input.npy",
                                                  "parameters.npy", "targets.npy"]
    assert total <= bench.DUMP_BYTES
    assert np.abs(np.load(tmp_path / "a" / "targets.npy")).max() > 0
