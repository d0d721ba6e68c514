"""bench.py's command line and its --dump-outputs writer, on the host (no GPU: the timed path itself runs under `-m gpu` and on the GPU box)."""
import numpy as np
import pytest
import torch
import bench


def test_plain_run_is_lean_by_default():
    a = bench.parse(['--gpus', '1', '--steps', '7', '--warmup', '2'])
    assert (a.steps, a.warmup, a.full, a.dump_outputs) == (7, 2, False, None)
    a = bench.parse(['--full', '--dump-outputs', 'out'])
    assert a.full and a.dump_outputs == 'out'


def test_stream_outputs_are_float_arrays_of_the_last_step(tmp_path):
    allsc = torch.rand(1, 2, 5, 2)
    results = [dict(response_token_ids=[[3, 4, 5], [6]], final_kv_len=120), dict(response_token_ids=[], final_kv_len=80)]
    out = bench.stream_outputs(allsc, results)
    bench.dump_outputs(str(tmp_path / 'd'), out)
    got = {k: np.load(tmp_path / 'd' / f'{k}.npy') for k in ('scores', 'response_token_ids', 'final_kv_len')}
    assert got['scores'].dtype == np.float32 and np.array_equal(got['scores'], allsc.numpy())
    assert got['response_token_ids'].dtype == np.float64 and got['response_token_ids'].shape == (2, 2, 3)
    assert got['response_token_ids'][0].tolist() == [[3, 4, 5], [6, -1, -1]] and (got['response_token_ids'][1] == -1).all()
    assert got['final_kv_len'].tolist() == [120.0, 80.0]


def test_dump_refuses_integer_arrays_and_oversize(tmp_path):
    with pytest.raises(AssertionError):
        bench.dump_outputs(str(tmp_path), {'ids': np.zeros(3, dtype=np.int64)})
    with pytest.raises(AssertionError):
        bench.dump_outputs(str(tmp_path), {'big': np.zeros(bench.DUMP_LIMIT_BYTES // 8 + 1, dtype=np.float64)})
