"""trtx_host_build, every family: the serialized plan is the recorded one byte for byte, and every refused call answers the recorded status
(tests/host_plan_cases.py).  The digests were recorded before the host builders were moved onto one block library, one build session and
one family table, from the commit named in tests/golden/host_plan_digests.json; they hold for every later change to those shared pieces.
CPU only.
"""
import hashlib

import pytest

import host_plan_cases as hp


@pytest.mark.parametrize("case", list(hp.PLAN_CASES))
def test_host_plan_is_the_recorded_plan(case, monkeypatch):
    monkeypatch.setenv("TRTX_TUNE", "0")
    gold = hp.load_golden()["plans"][case]
    if hp.wts_sha(case) != gold["wts_sha256"]:
        pytest.skip("the seeded synthetic weights differ from the ones the digest was recorded on (different torch build)")
    plan = hp.build(case)
    assert len(plan) == gold["plan_bytes"]
    assert hashlib.sha256(plan).hexdigest() == gold["plan_sha256"]


def test_every_recorded_plan_has_a_case_and_a_parent():
    gold = hp.load_golden()
    assert sorted(gold["plans"]) == sorted(hp.PLAN_CASES)
    assert len(gold["recorded_from_commit"]) == 40


@pytest.mark.parametrize("model,opts,wts,status", hp.STATUS_CASES,
                         ids=[f"{m}-{'-'.join(f'{k}{v}' for k, v in o.items()) or 'defaults'}-{w[0]}" for m, o, w, _ in hp.STATUS_CASES])
def test_host_build_status(model, opts, wts, status):
    assert hp.status_of(model, opts, wts) == status
