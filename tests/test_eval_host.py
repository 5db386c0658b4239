"""CPU-side checks of the evaluation surface: the result summary and the argument checks that need no GPU."""
import numpy as np
import pytest

from dqnflappybird_amd import _lib as L
from dqnflappybird_amd.evaluate import EvalResult, evaluate


def test_summary_statistics():
    score = np.array([[3, 0], [10, 5], [0, 0]], np.int32)
    length = np.array([[120, 0], [400, 90], [50, 0]], np.int32)
    trunc = np.array([[0, 0], [0, 1], [1, 0]], np.uint8)
    r = EvalResult(score, length, trunc, steps=490, wall_s=2.0, rows_launched=700)
    s = np.array([3, 10, 5, 0], float)                       # recorded entries only (length > 0)
    assert r.episodes == 4 and r.truncated_count == 2
    assert r.env_steps == 660 and r.env_steps_per_s == 330.0
    assert r.mean_score == s.mean() and r.median_score == np.median(s) and r.max_score == 10
    assert r.p10_score == np.percentile(s, 10) and r.p90_score == np.percentile(s, 90)
    assert r.mean_length == 165.0 and r.rows_per_live_row == 700 / 660
    line = r.summary()
    assert line.startswith("EVAL ENVS 3 / EPISODES 4 / TRUNCATED 2 / MEAN_SCORE 4.500") and "STEPS 490" in line


def test_empty_result():
    z = np.zeros((2, 1), np.int32)
    r = EvalResult(z, z, np.zeros((2, 1), np.uint8), steps=1, wall_s=0.1)
    assert r.episodes == 0 and np.isnan(r.mean_score) and r.max_score == 0


@pytest.mark.parametrize("n", [0, L.EVAL_MAX_ENVS + 1])
def test_env_count_is_checked_first(n):
    with pytest.raises(ValueError):
        evaluate(object(), n)


def test_header_limits_match_the_binding():
    import os
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "fbdqn.h")).read()
    assert f"#define FB_EVAL_MAX_ENVS {L.EVAL_MAX_ENVS}" in text and f"#define FB_EVAL_MAX_EPISODES {L.EVAL_MAX_EPISODES}" in text
