"""-m gpu: every kernel instance the library lists runs against the oracle, and the launch tally shows that it ran.

pick_route() (iac_amd/csrc/render_route.hpp) chooses one of several hundred exact kernels per call and the general
kernel takes whatever the others refuse, so a parity test passes whichever kernel ran.  Each case of tests/route_cases.py
resets the library's tally (iamf_hip_route_tally), makes the smallest calls that reach its instance — three streams,
three calls with the state carried over, the flush — and asserts both the instances launched and the result.
tests/test_route_coverage_cpu.py holds the cases against the library's listing."""
import pytest

import route_cases as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def gpu():
    import torch
    assert torch.cuda.is_available()


@pytest.mark.parametrize("case", R.CASES, ids=[c.id for c in R.CASES])
def test_instance_runs_and_matches_the_oracle(case, monkeypatch):
    for k in ("IAMF_HIP_FORCE_GENERIC", "IAMF_HIP_NO_WIDE4", "IAMF_HIP_PROJECTION", "IAMF_HIP_LP_LATE", "IAMF_HIP_LPCM_UNFUSED",
              "IAMF_HIP_FIR_FUSED", "IAMF_HIP_FIR_F16", "IAMF_HIP_FIR_F32", "IAMF_HIP_RESAMPLE_TILE", "IAMF_HIP_RESAMPLE_PLAIN"):
        if k not in case.kw.get("env", {}) and k != "IAMF_HIP_FORCE_GENERIC":
            monkeypatch.delenv(k, raising=False)
    case.build(case)


@pytest.mark.parametrize("case", R.UNREACHABLE, ids=[u.id for u in R.UNREACHABLE])
def test_nearest_call_of_an_unreachable_instance_is_routed_elsewhere(case):
    """the call that would take the instance if its launcher's rule let it: it matches the oracle on the kernel the rule
    names instead (kw["routed"]), and the instance's own counter stays at zero"""
    import iac_amd as A
    case.build(case)                      # asserts the tally is exactly {routed: calls}
    assert case.inst not in A.route_tally(reset=False)
