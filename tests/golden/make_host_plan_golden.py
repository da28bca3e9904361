"""Writes tests/golden/host_plan_digests.json: for every case of tests/host_plan_cases.py the SHA-256 and size of the plan trtx_host_build
serializes (TRTX_TUNE=0) and the SHA-256 of the seeded weights file it was built from, plus the commit whose build recorded them.  Run it
from the repository root on a build of the commit that is to be the specification:
    python tests/golden/make_host_plan_golden.py <commit hash>
"""
import hashlib
import json
import os
import sys

os.environ["TRTX_TUNE"] = "0"
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import host_plan_cases as hp  # noqa: E402

commit = sys.argv[1]
assert len(commit) == 40, "the full hash of the commit whose build is recorded"
plans = {}
for case in hp.PLAN_CASES:
    plan = hp.build(case)
    plans[case] = {"plan_sha256": hashlib.sha256(plan).hexdigest(), "plan_bytes": len(plan), "wts_sha256": hp.wts_sha(case)}
    print(case, plans[case], flush=True)
with open(hp.GOLDEN, "w") as f:
    json.dump({"recorded_from_commit": commit, "plans": plans}, f, indent=1, sort_keys=True)
    f.write("\n")
