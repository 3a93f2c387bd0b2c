"""Status and mdvt_last_error text of every wrong call of tests/refusal_cases.py, compared exactly with
tests/golden/refusal_text.json: the texts Python callers read inside MdvtError, and -- through the pairs of wrong arguments -- the
order of every entry point's checks.  The golden file was recorded with the library as it was before this test existed, so any
tidying of csrc/mdvt_api.hip since then is held to it.  The test provokes nothing: every case returns from
host code before a launch, or is an ordinary small call."""
import pytest

import refusal_cases as rc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def answers():
    return rc.run_all()


def test_every_case_answers_as_recorded(answers):
    golden = rc.load_golden()
    assert list(answers) == list(golden)
    wrong = []
    for name, cases in answers.items():
        assert list(cases) == list(golden[name]), name
        wrong += [f"{name} [{label}]: {tuple(got)} -- recorded {tuple(golden[name][label])}" for label, got in cases.items()
                  if tuple(got) != tuple(golden[name][label])]
    assert not wrong, f"{len(wrong)} answer(s) changed:\n" + "\n".join(wrong[:40])


def test_the_cases_reach_the_refusals(answers):
    """The table is worth its name: about a thousand calls, most of them refused, every ctx entry point with at least the two texts
    each of them has (a NULL buffer, a pitch or stride below its row or frame)."""
    n = sum(len(c) for c in answers.values())
    refused = sum(1 for c in answers.values() for status, _ in c.values() if status != 0)
    assert n >= 900 and refused >= n // 2
    for e in rc.TABLE:
        if "ctx" in e.by_name:
            texts = {text for status, text in answers[e.name].values() if status != 0}
            assert len(texts) >= 2 and "" not in texts, e.name
