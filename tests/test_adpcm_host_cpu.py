"""The kernels of csrc/vv_adpcm.hip (N25) compiled for the host and run under sanitizers (tools/adpcm_host_check.{cpp,py}): one OS thread
per GPU thread, every buffer an exact-size heap block, the results compared with the mirror the GPU tests use.  Two builds: ``asan``
(-fsanitize=address,undefined) and ``tsan`` (-fsanitize=thread).  Each runs the tool's reduced list, which keeps every edge and drops the
bulk; the full list is ``python tools/adpcm_host_check.py``.  The program is stand-alone: nothing is loaded into this process under a
sanitizer.  Needs no GPU."""
import pytest

from tests.host_check_util import tool


@pytest.mark.parametrize("san", ("asan", "tsan"))
def test_adpcm_kernels_on_the_shim_equal_the_mirror_with_no_report(san, tmp_path):
    t = tool("adpcm")
    cxx = t.find_cxx()
    if cxx is None:
        pytest.skip("no host C++ compiler found")
    exe = t.build(cxx, str(tmp_path), san)
    res = list(t.cases(exe, str(tmp_path), reduced=True))            # a sanitizer report, a non-zero exit or a run past its time limit raises
    assert len(res) >= 20 and not [label for label, ok in res if not ok]
