"""bench.py's command line: a plain run times exactly --steps steps and reports the headline alone, --dump-outputs
writes the records the last timed step returned (the seeded workload's own records, bit for bit), --full adds the
profile, the roofline and the accuracy."""
import json

import numpy as np
import pytest

SMALL = ["--gpus", "1", "--steps", "3", "--warmup", "1", "--frags", "4", "--npts", "1000"]
FULL_ONLY = ("roofline", "cpu_baseline", "accuracy", "secondary")


def _line(capsys):
    return json.loads(capsys.readouterr().out.strip().splitlines()[-1])


def test_prof_seq_needs_full(tmp_path):
    import bench
    with pytest.raises(SystemExit) as e:
        bench.main(SMALL + ["--prof-seq", str(tmp_path / "seq.json")])
    assert e.value.code == 2


@pytest.mark.gpu
def test_plain_run_headline_and_dump(gpu, tmp_path, capsys):
    import torch
    import bench
    bench.main(SMALL + ["--dump-outputs", str(tmp_path / "out")])
    line = _line(capsys)
    assert line["steps"] == 3 and line["warmup"] == 1 and line["n_gpus"] == 1
    assert line["unit"] == "pairs/s" and line["higher_is_better"] is True and line["dtype"].startswith("f32")
    assert line["ms_per_step"] > 0
    # 6 pairs per step: value and ms_per_step are the same measurement (both rounded to 3 decimals)
    assert abs(line["value"] * line["ms_per_step"] / 6e3 - 1) < 1e-3
    assert all(line[k] is None for k in FULL_ONLY)
    rec = np.load(tmp_path / "out" / "records.npy")
    assert rec.dtype == np.float32 and rec.shape == (6, 13)
    with torch.no_grad():
        ref = bench.SceneWorkload(gpu, 0, npts=1000, n_frag=4).step()
    assert np.array_equal(rec, ref.cpu().numpy())


@pytest.mark.gpu
def test_full_run_adds_profile_and_accuracy(gpu, capsys):
    import bench
    bench.main(SMALL + ["--full", "--no-cpu-baseline", "--no-secondary"])
    line = _line(capsys)
    assert line["steps"] == 3 and line["ms_per_step"] > 0
    assert line["roofline"]["kernel"] in line["roofline"]["classes"]
    assert line["roofline"]["whole_step"]["ms_per_step"] == line["ms_per_step"]
    assert line["accuracy"]["pair_blocks_over_1e-4"] == 0 and line["accuracy"]["mask_mismatches_vs_ref"] == 0
    assert line["cpu_baseline"] is None and line["secondary"] is None
