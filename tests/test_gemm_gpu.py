"""-m gpu: the GEMM kernels of vv_gemm.hip (gemm_kernel<f32 / bf16> in its 128, 256 (16 waves), 64 x 128 and 64 x 64 ring forms, the
persistent gemm_pp_kernel with both of its store paths, the split-K tail) against float64 references of the operands as given, element
by element.

Reference (tests/gpu_util.py gemm_ref): z = A W^T + bias in float64; MODE_STORE f(z); MODE_QKV_ROPE interleaved pairs
(a, b) -> (a c - b s, b c + a s) on columns [rope_lo, 2 rope_dim) with c, s from the fp32 tables at rope_pos[m] (or m % seq_n), or float64
cos / sin of pos theta^(-2i/64) in the computed form; MODE_GATE_RES x0 + gate z (or x0 + z); MODE_GATE_STORE gate z.  Metric: err = max_e
(|got_e - ref_e| - allow_e) / A_e, A_e the same expression on absolute values (an activation: 1.13 A_z).  Bound: max(8 x 2^-24, 4 x yardstick),
yardstick = the CPU library in fp32 on the same operands.  Allowances per element: a bf16 output its store rounding 2^-8 |ref_e|; an
activation 8 x 2^-24 |z_e|; the computed rope 4 (kappa 2^-24 angle + theta0) (|a| + |b|) with kappa, theta0 measured on the CPU
(gpu_util.rope_angle_model).  Every case also keeps the old whole-tensor tolerance.  One GEMM_PARITY line per case;
profiles/gemm_parity/notes.md records them.

Every launch goes through gpu_util.gemm_launch: C is a view inside a buffer of 7.0 with 64 guard rows in front and behind and (padded
run) 8 / 4 padding columns, A and W are views with lda = K + 8 and ldw = K + 16 whose padding and the rows behind hold NaN, bias and gate
are followed by NaN; the guards are checked after the launch; each case runs contiguous and padded and the two outputs must be the same
bits.  The cases and the kernel each one claims to reach are listed in gpu_util.gemm_cases(); tests/test_gemm_ref_cpu.py checks the claims
against a restatement of launch()."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import gpu_util as gu  # noqa: E402
from vietvoice_tts_amd import runtime as rt  # noqa: E402

CASES = gu.gemm_cases()
WALK = gu.gemm_walk_cases()


def _ids(cases):
    return [c.name for c in cases]


def _bits_equal(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(torch.int16), b.contiguous().view(torch.int16))


def _old_tolerance(case):
    """The whole-tensor limits of tests/test_kernels_gpu.py: fp32 2e-4, bf16 1.5e-2, bf16 operands with fp32 output 1e-3 (2e-3 on the
    residual stream)."""
    if not case.bf16_in:
        return gu.TOL_F32
    if not case.out_f32:
        return gu.TOL_BF16
    return 2e-3 if case.mode == gu.MODE_GATE_RES else 1e-3


def _check(case, got, misses, tag=""):
    """Parity of one output of a case (columns below n_store), the fill from n_store rounded up to the store quantum on, the old tolerance;
    prints the GEMM_PARITY line."""
    r = case.refs()
    lo, hi = gu.gemm_written_cols(case)
    assert got.shape == r.ref.shape
    err, where = gu.parity_err(got[:, :lo], r.ref[:, :lo], r.A[:, :lo], r.allow[:, :lo])
    old = gu.rel_err(got[:, :lo], r.ref[:, :lo])
    print(f"\nGEMM_PARITY case={case.name}{tag} kernel={case.kernel} err={err:.3e} yardstick={r.yard:.3e} bound={r.bound:.3e} ratio={err / r.bound:.2f} "
          f"old_rel_err={old:.2e} worst_row_col={where}")
    if case.rope == "computed":         # how much of the angle model (kappa 2^-24 angle + theta0, WITHOUT the factor 4) the device needs beyond the other terms
        o, D = case.ops(), case.rope_dim
        kappa, theta0 = gu.rope_angle_model()
        model = (r.allow - gu.BF16_STORE * r.ref.abs())[:, :2 * D] / gu.ROPE_FACTOR
        over = ((got.double() - r.ref).abs() - gu.BF16_STORE * r.ref.abs() - r.bound * r.A)[:, :2 * D].clamp_min(0.0)
        ratio = torch.where(model > 0, over / model.clamp_min(1e-300), torch.zeros_like(over))
        i = int(ratio.argmax())
        print(f"GEMM_ROPE_ANGLE case={case.name}{tag} kappa={kappa:.2f} theta0={theta0:.1e} device_excess/angle_model={float(ratio.max()):.3f} "
              f"at row {i // (2 * D)} (position {int(o.pos[i // (2 * D)])}), column {i % (2 * D)}; allowed {gu.ROPE_FACTOR:.0f}")
    if not err <= r.bound:
        misses.append((case.name + tag, f"err {err:.3e} > bound {r.bound:.3e} at (row, column) {where}: got {float(got[where]):.9g}, ref {float(r.ref[where]):.9g}"))
    if not old < _old_tolerance(case):
        misses.append((case.name + tag, f"whole-tensor rel_err {old:.3e} >= {_old_tolerance(case)}"))
    if hi < case.N and not bool((got[:, hi:].float() == gu.CONV_FILL).all()):
        bad = (got[:, hi:].float() != gu.CONV_FILL).nonzero()[0].tolist()
        misses.append((case.name + tag, f"a column at or past n_store rounded up ({hi}) was written: (row, column - {hi}) {bad}"))


@pytest.mark.parametrize("case", CASES, ids=_ids(CASES))
def test_gemm_float64_parity(hip_tiny, case):
    """Every case of the grid: per element against float64 inside the derived bound, inside the old whole-tensor tolerance, guard rows
    and padding columns intact, the padded launch bit-identical to the contiguous one; the other bf16 tilings of the case (twins) and
    the automatic choice (tile = 0 against the forced tile the dispatch rule names) bit-identical too."""
    eng = hip_tiny["f32"]
    misses = []
    plain = gu.gemm_launch(eng, case, padded=False)
    padded = gu.gemm_launch(eng, case, padded=True)
    _check(case, plain, misses)
    if not _bits_equal(plain, padded):
        d = (plain.float() != padded.float()).nonzero()
        misses.append((case.name, f"the padded launch differs from the contiguous one at {d[0].tolist() if len(d) else 'NaN bits'}"))
    for t in case.twins + ((gu._TILE_OF_KERNEL[case.kernel],) if case.tile == 0 else ()):
        twin = gu.gemm_launch(eng, case, padded=True, tile=t)
        if not _bits_equal(twin, padded):
            d = (twin.float() != padded.float()).nonzero()
            misses.append((case.name, f"tile {t} differs from tile {case.tile} at {d[0].tolist() if len(d) else 'NaN bits'} ({len(d)} elements)"))
    assert not misses, misses


@pytest.mark.parametrize("case", WALK, ids=_ids(WALK))
def test_gemm_persistent_workgroup_walks_on_whole_output(hip_tiny, case):
    """602 tiles on the chip's workgroups: every workgroup of the persistent kernel walks two or three tiles and the last round is
    partial.  The WHOLE output per element, contiguous and padded."""
    eng = hip_tiny["f32"]
    misses = []
    plain = gu.gemm_launch(eng, case, padded=False)
    _check(case, plain, misses)
    padded = gu.gemm_launch(eng, case, padded=True)
    assert _bits_equal(plain, padded), "the padded launch differs from the contiguous one"
    assert not misses, misses


def test_gemm_split_k_tail_float64_parity(hip_tiny):
    """The split-K tail (N = 512, K = 512, 136 panels less 100 rows): the fp32 K parts of the tail rows summed in float64 under the fp32
    bound (no store term: nothing was rounded to bf16), the first and the last main panel under the bf16 bound; C's tail rows, the
    padding columns of the parts and the guards keep their fill."""
    eng = hip_tiny["f32"]
    case = gu.gemm_tail_case()
    M, N, K = case.M, case.N, case.K
    row0, parts = gu.gemm_tail_plan(eng, M, N, K)
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count // 8 * 8
    assert case.m_tiles * (N // 256) % n_cu != 0 and parts == 4 and row0 % 2048 == 0 and 0 < row0 < M, (row0, parts, n_cu)
    r = case.refs()
    misses = []
    for padded in (False, True):
        ldc = case.ld(padded)[2]
        Ct = torch.full((parts, M - row0, ldc), gu.CONV_FILL, dtype=torch.float32, device=gu.DEV)
        got = gu.gemm_launch(eng, case, padded=padded, tail=(Ct, row0, parts))
        assert bool((got[row0:].float() == gu.CONV_FILL).all()), "the tail rows of C are left to the consumer"
        ct = Ct.cpu()
        assert bool((ct[:, :, N:] == gu.CONV_FILL).all()), "padding columns of the tail parts were written"
        total = ct[:, :, :N].double().sum(0)
        err, where = gu.parity_err(total, r.ref[row0:], r.A[row0:])
        print(f"\nGEMM_PARITY case={case.name}/tail_rows{'/padded' if padded else ''} kernel={case.kernel} err={err:.3e} yardstick={r.yard:.3e} bound={r.bound:.3e} "
              f"ratio={err / r.bound:.2f} old_rel_err={gu.rel_err(total, r.ref[row0:]):.2e} worst_row_col={where}")
        if not err <= r.bound:
            misses.append(("tail rows", padded, err, where))
        for name, rows in (("first_panel", slice(0, 256)), ("last_main_panel", slice(row0 - 256, row0))):
            err, where = gu.parity_err(got[rows], r.ref[rows], r.A[rows], r.allow[rows])
            old = gu.rel_err(got[rows], r.ref[rows])
            print(f"\nGEMM_PARITY case={case.name}/{name}{'/padded' if padded else ''} kernel={case.kernel} err={err:.3e} yardstick={r.yard:.3e} bound={r.bound:.3e} "
                  f"ratio={err / r.bound:.2f} old_rel_err={old:.2e} worst_row_col={where}")
            if not (err <= r.bound and old < gu.TOL_BF16):
                misses.append((name, padded, err, old, where))
    assert not misses, misses


def _raw_args(case, Cv, A, W, bias, gate=None):
    a = rt.vv_gemm_args()
    a.dtype = rt.VV_BF16 if case.bf16_in else rt.VV_F32
    a.out_dtype = rt.VV_F32 if case.out_f32 else rt.VV_BF16
    a.A, a.lda, a.W, a.ldw, a.C, a.ldc = A.data_ptr(), A.stride(0), W.data_ptr(), W.stride(0), Cv.data_ptr(), Cv.stride(0)
    a.M, a.N, a.K, a.bias, a.tile = case.M, case.N, case.K, bias.data_ptr(), case.tile
    a.gate = None if gate is None else gate.data_ptr()
    return a


def test_gemm_n_store_is_for_the_plain_store_only(hip_tiny):
    """include/vvtts.h: n_store applies to VV_EPI_STORE; vv_gemm refuses a non-zero n_store in every other mode (-22) and launches
    nothing.  (What a plain store with n_store writes is checked per element by the n_store cases of the grid: columns below n_store are
    right, columns from n_store rounded up to 4 (8 for bf16 output) on keep their fill.)"""
    eng = hip_tiny["f32"]
    by_name = {c.name: c for c in CASES}
    for name in ("f32_128_gate_store", "bf16_128_gate_store", "pp_gate_store", "pp_gate_res", "f32_256_res_ungated", "pp_rope_tables", "bf16_64_rope_tables"):
        case = by_name[name]
        o = case.ops()
        A, W, bias, gate = o.A.to(gu.DEV), o.W.to(gu.DEV), o.bias.to(gu.DEV), o.gate.to(gu.DEV)
        Cv = torch.full((case.M, case.N), gu.CONV_FILL, dtype=case.out_dtype, device=gu.DEV)
        a = _raw_args(case, Cv, A, W, bias, gate)
        a.mode, a.n_store = case.mode, 100
        if case.mode == gu.MODE_QKV_ROPE:
            tabs = [t.to(gu.DEV) for t in o.tables]
            a.cos_q, a.sin_q, a.cos_k, a.sin_k = [t.data_ptr() for t in tabs]
            a.seq_n, a.rope_dim = case.seq_n, case.rope_dim
        rc = eng.lib.vv_gemm(eng.ctx, C.byref(a), gu.stream())
        torch.cuda.synchronize()
        assert rc == -22 and b"n_store" in eng.lib.vv_last_error(eng.ctx), (name, rc, eng.lib.vv_last_error(eng.ctx))
        assert bool((Cv.float() == gu.CONV_FILL).all()), (name, "a refused call wrote to C")
