"""GPU: every kernel path of the set operations, pinned.  For each case of tests/path_cases.py the call must show exactly the
expected delta of Context.paths() - the kernels, template instantiations and kernel sequences it launched - and return the plain
numpy reference bit for bit; with the lists in one segment, spread over two, and (where the case says so) in a segment of 65537
lists, whose doc spans the host does not mirror: there the delta also names the span fetches and bounds reductions, and a repeat
of the call fetches no span again."""
import pytest

from tests import path_cases as pc
from tests.gpu_util import ctx, run_path_case  # noqa: F401

pytestmark = pytest.mark.gpu

CASE_LAYOUTS = [pytest.param(case, layout, id=f"{case.name}-{layout}") for case in pc.CASES for layout in case.layouts()]


@pytest.mark.parametrize("case,layout", CASE_LAYOUTS)
def test_path_and_result(ctx, case, layout):
    run_path_case(ctx, case, layout, pc.DEFAULTS)
