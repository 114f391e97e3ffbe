"""Writes the launch table of tests/launch_table_cases.py as JSON (default: tests/golden/launch_table_parent.json).

    python tests/golden/make_golden_launch_table.py [out.json]

The committed file was recorded on an MI355X at the commit BEFORE the native launch got its one definition
(sceneverse_amd/_launch.py): tests/test_gpu_launch_table.py holds every later commit to the same launches, profile keys and
per-launch accounting.  Regenerate it only with a change that is meant to alter the set of launches."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from launch_table_cases import GOLDEN, launch_table  # noqa: E402

if __name__ == "__main__":
    out = sys.argv[1] if len(sys.argv) > 1 else GOLDEN
    table = launch_table("cuda")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(table, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"{len(table)} profile keys, {sum(v['launches'] for v in table.values())} launches -> {out}")
