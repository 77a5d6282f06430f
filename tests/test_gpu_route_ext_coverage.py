"""-m gpu: every kernel instance of the library's extension table runs against the oracle, and the extension tally shows
that it ran (tests/route_cases_ext.py; tests/test_route_ext_coverage_cpu.py holds the cases against the listing)."""
import pytest

import route_cases_ext as RX

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def gpu():
    import torch
    assert torch.cuda.is_available()


@pytest.mark.parametrize("case", RX.CASES, ids=[c.id for c in RX.CASES])
def test_ext_instance_runs_and_matches_the_oracle(case, monkeypatch):
    for k in ("IAMF_HIP_FORCE_GENERIC", "IAMF_HIP_LP_LATE", "IAMF_HIP_LPCM_UNFUSED"):
        monkeypatch.delenv(k, raising=False)
    case.build(case)
