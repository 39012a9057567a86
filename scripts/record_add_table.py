"""Records tests/golden/add_table.json: what every case of tests/add_table_cases.py gives on the commit it is run on (needs the GPU).  The table
pins the add family's behaviour across a rework of the add path, so it is taken from the commit BEFORE that rework and never from the code it is
to check: python scripts/record_add_table.py <commit hash> [output file]"""
import json
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import add_table_cases as T  # noqa: E402


def main():
    commit = sys.argv[1]
    out = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "tests", "golden", "add_table.json")
    table = {}
    with tempfile.TemporaryDirectory() as base:
        runner = T.Runner(os.path.join(ROOT, "tests", "golden", "jpeg_ref.npz"), base)
        try:
            for case in T.CASES:
                for name, via in T.runs(case, with_entry=False):       # (l3d_line3d_add_image_entry is checked against these records)
                    table[name + "/" + via] = runner.run(case, via)
        finally:
            runner.close()
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        json.dump(dict(commit=commit, records=table), f, indent=1, sort_keys=True)
        f.write("\n")
    print("%d records of %d cases written to %s" % (len(table), len(T.CASES), out))


if __name__ == "__main__":
    main()
