"""-m gpu: state hand-over between every pair of render kernel families that can meet on one batch.

render_route.hpp says of the families that "all share the persisted per-stream state, so consecutive calls of one stream may
take different ones"; every family restores and saves LimState, d_ring_y, d_ring_pm (and d_lfe_state) in its own code.  A
case (tests/handover_util.py) is (class, A, B, b): family A renders call 1 of b samples, family B renders call 2,
iamf_hip_batch_flush ends the stream.  490 cases over 12 batch classes, every ordered pair of a class at every boundary b
in 1024, 1088, 1280, 1000 at which A can end and B can start, and one case per class at b = 100; 6 streams per batch, one
limiter phase per stream at the boundary (idle, look-ahead, mid-attack, release, re-trigger, edge — proven from the oracle's
limiter trace in tests/test_handover_cpu.py).

Every case asserts, tolerance 0 (class WM, the MFMA projection: +-1 LSB and no state comparison):
  tallies      the base table, the extension table, table 2 and the by-family listings together hold exactly one launch of
               the expected family's row per call and member, and one GENERIC row per member for the flush; nothing else
  PCM          call 1, call 2 and the flush, per stream, equal the oracle's bytes
  shapes       the values returned: b - 240, the length of call 2 and 240 (less what the delay still holds at b = 100)
  stray writes every PCM byte outside the emitted runs is still 0xA5 (gpu_util.rows_and_rest)
  state        after call 1 and after call 2 the blob and the tickets of iamf_hip_batch_export_range equal, bit for bit,
               those of a control batch that ran the same calls through iamf_hip_batch_render_range under
               IAMF_HIP_FORCE_GENERIC=1 (the saved rings are canonical).  This names the call that WROTE bad
               state, not the later one that read it.  No entry of the blob is masked (handover_util.state_mask).
In a case that names a fan-out family both member batches are checked.

One test id runs all of them, group by group — a group is (class, A), 38 of them — and case by case (each_case, as in
tests/test_gpu_ragged.py): a failed assertion is kept and the next case runs, the test fails with the list, every entry under
its group; any other exception — a HIP error — ends the test at once.  The whole takes a few seconds."""
import pytest

import handover_util as H

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def gpu():
    import torch
    assert torch.cuda.is_available()


@pytest.fixture(autouse=True)
def clean_switches(monkeypatch):
    for k in H.SWITCHES:
        monkeypatch.delenv(k, raising=False)


def each_case(cases, fn):
    """fn(case) for every case; an assertion that fails is kept and the next case runs -> the list of what failed.  (Any
    other exception — a HIP error — is not caught: it ends the test at once.)"""
    failed = []
    for case in cases:
        try:
            fn(case)
        except AssertionError as e:
            failed.append("%s: %s" % (H.case_id(case), e))
    return failed


def test_handover():
    groups = H.groups()
    assert len(groups) == 38 and sum(len(v) for v in groups.values()) == H.N_CASES
    report, n_failed = [], 0
    for (cls, a), cases in sorted(groups.items()):
        failed = each_case(cases, H.check_case)
        if failed:
            n_failed += len(failed)
            report.append("[%s, A = %s] %d of %d cases failed:\n%s" % (cls, a, len(failed), len(cases), "\n".join(failed)))
    assert not report, "%d of %d cases failed:\n%s" % (n_failed, H.N_CASES, "\n".join(report))
