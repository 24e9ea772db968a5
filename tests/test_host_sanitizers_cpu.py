"""The PCM-stage, ingest and edit kernels compiled for the host and run under sanitizers (tools/*_host_check.{cpp,py}): one OS thread per
GPU thread, every buffer an exact-size heap block, the results compared with the mirrors the GPU tests use.  Per kernel file two builds:
``asan`` (-fsanitize=address,undefined: an index past an end, a misaligned vector access) and ``tsan`` (-fsanitize=thread: an LDS write
and a read with no barrier between).  Each runs the tool's reduced list, which keeps every edge and drops the bulk; the full lists are
``python tools/X_host_check.py``.  The programs are stand-alone: nothing is loaded into this process under a sanitizer.  Needs no GPU."""
import pytest

from tests.host_check_util import NEW, OLD, tool

BUILDS = ("asan", "tsan")


def _cxx(t):
    cxx = t.find_cxx() if hasattr(t, "find_cxx") else tool("flac_decode").find_cxx()
    if cxx is None:
        pytest.skip("no host C++ compiler found")
    return cxx


@pytest.mark.parametrize("san", BUILDS)
@pytest.mark.parametrize("name", NEW)
def test_kernels_on_the_shim_equal_the_mirror_with_no_report(name, san, tmp_path):
    t = tool(name)
    exe = t.build(_cxx(t), str(tmp_path), san)
    res = list(t.cases(exe, str(tmp_path), reduced=True))            # a sanitizer report, a non-zero exit or a run past its time limit raises
    assert len(res) >= 4 and not [label for label, ok in res if not ok]


@pytest.mark.parametrize("san", BUILDS)
def test_flac_decode_kernels_equal_the_mirror_with_no_report(san, tmp_path):
    from tests import flac_decode_util as U
    t = tool("flac_decode")
    exe = t.build(_cxx(t), str(tmp_path), san)
    n, skipped, bad = t.run(exe, str(tmp_path), [(c[0], c[1]) for c in U.cases()][::4] + [(m[0], m[1]) for m in U.malformed()])
    assert n > 30 and not bad


@pytest.mark.parametrize("san", BUILDS)
@pytest.mark.parametrize("name", [n for n in OLD if n != "flac_decode"])
def test_kernels_on_their_own_stand_ins_equal_the_mirror_with_no_report(name, san, tmp_path, capsys):
    t = tool(name)
    _cxx(t)
    try:
        t.main(["--san", san, "--keep", str(tmp_path), "--reduced"])  # raises SystemExit on a difference, a report or a non-zero exit
    except SystemExit as e:
        pytest.fail(f"tools/{name}_host_check.py --san {san} --reduced: {e.code}\n{capsys.readouterr().out[-2000:]}")
    assert "ok: the kernels equal the mirror" in capsys.readouterr().out
