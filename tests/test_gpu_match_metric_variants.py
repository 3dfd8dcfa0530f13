"""tests/test_gpu_match_metric.py again under the library's other knob settings.  The library reads its knobs once per process, so each setting runs
the file in a fresh CHILD python (subprocess.run: a child, never an exec of this GPU-initialised process), one after the other, each with its own
timeout, as tests/test_gpu_variants.py does for the euclidean files:

  KPB_MATCH_PREFILTER=0  match_tile<.., METRIC> on every pair of every metric;
  KPB_MATCH_PREFILTER=2  the prefilter for ANY number of pairs where the metric has one (sqeuclidean: euclidean's; cosine: its own): the calls of
                         three and five pairs and the Python layers' single pairs then take it too;
  KPB_FP32_MATRIX=1      the strict-fp32 network kernels (the matcher reads no such knob: its bits must not move).

Every setting is held to the same expectation, hence to the same bits.  A child that failed is not started again, and no further child is started
after it: the remaining settings fail at once."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_FAILED = []


@pytest.mark.timeout(400)
@pytest.mark.parametrize("knob", ["KPB_MATCH_PREFILTER=0", "KPB_MATCH_PREFILTER=2", "KPB_FP32_MATRIX=1"])
def test_the_metric_tests_under_the_other_settings(knob):
    assert not _FAILED, "not started: the child under %s failed" % _FAILED[0]
    name, value = knob.split("=")
    cmd = [sys.executable, "-m", "pytest", "-x", "-q", "-m", "gpu", "-p", "no:cacheprovider", "tests/test_gpu_match_metric.py"]
    _FAILED.append(knob)
    p = subprocess.run(cmd, cwd=ROOT, env=dict(os.environ, **{name: value}), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=360)
    tail = "\n".join(p.stdout.splitlines()[-25:])
    assert p.returncode == 0, "child pytest with %s failed:\n%s" % (knob, tail)
    assert " passed" in tail and "skipped" not in tail.split("passed")[-1], tail
    _FAILED.remove(knob)
