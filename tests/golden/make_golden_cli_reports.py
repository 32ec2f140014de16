"""Records tests/golden/cli_reports.json: what every run of tests/test_cli_reports_cpu.py writes today -- the files of the
output directory, every .csv, run_headers(param).  These are this project's own outputs over the test's seeded counter, so
the file is recorded once, from the commit whose reports are to be kept, and again only when a report changes on purpose:

    python tests/golden/make_golden_cli_reports.py
"""
import json
import os
import sys
import tempfile

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]

import test_cli_reports_cpu as T  # noqa: E402


def main():
    recorded = {}
    for run in T.RUNS:
        with tempfile.TemporaryDirectory() as tmp, pytest.MonkeyPatch.context() as patch:
            patch.chdir(tmp)
            recorded[T.run_id(*run)] = T.run_cli(*run, patch)
    with open(T.GOLDEN_FILE, "w") as out:
        json.dump(recorded, out, indent=1, sort_keys=True)
        out.write("\n")
    print(f"{len(recorded)} runs -> {T.GOLDEN_FILE}")


if __name__ == "__main__":
    main()
