"""The batch codec's C entries answer as the recorded contract says (tests/batch_contract.py; tests/golden/batch_contract.json
holds the answers in the order of its case list, every message once): every refusal with its return code and its
jpegx_last_error() text byte for byte -- so also WHICH check answers when two would -- and every size, group_planes and groups function with its value, over all four families.  The record is of the commit
before the entries' shared host code moved into csrc/jpegx_batch_common.h.  CPU only: every recorded call is a pure host
function or is refused by an argument check before any HIP call (the recorder asserts it), so no device is touched."""
import json

import pytest

import batch_contract
import jpegx


@pytest.fixture(scope="module")
def answers():
    got = batch_contract.run(jpegx.lib())
    with open(batch_contract.GOLDEN) as f:
        want = batch_contract.unpack(json.load(f), list(got))      # asserts that the case list is the recorded one
    return want, got


def test_the_case_list_is_the_recorded_one(answers):
    want, got = answers
    assert sorted(got) == sorted(want)
    assert len(want) > 2500 and sum(1 for v in want.values() if isinstance(v, list) and len(v) == 2) > 1000


def test_every_refusal_answers_with_the_same_code_and_text(answers):
    want, got = answers
    refusals = [k for k, v in want.items() if isinstance(v, list) and len(v) == 2]
    wrong = {k: (want[k], got[k]) for k in refusals if got[k] != want[k]}
    assert not wrong, "%d of %d refusals differ, the first: %r" % (len(wrong), len(refusals), sorted(wrong.items())[:3])


def test_every_size_and_cut_is_the_same(answers):
    want, got = answers
    host = [k for k, v in want.items() if not (isinstance(v, list) and len(v) == 2)]
    wrong = {k: (want[k], got[k]) for k in host if got[k] != want[k]}
    assert not wrong, "%d of %d host answers differ, the first: %r" % (len(wrong), len(host), sorted(wrong.items())[:3])
