"""Check that every forward case of tests/test_launch_forms_gpu.py ran the aggregation form that
tests/launch_forms.py `expected_forms` names: the typed-aggregation kernel and its grid, and the grid of the bf16 twins'
scene-form launch, read from a kernel trace of those cases.

    rocprofv3 --kernel-trace --output-format csv -d <dir> -o kt -- \
        python -m pytest -m gpu tests/test_launch_forms_gpu.py -k forward -p no:cacheprovider
    python tools/launch_forms_trace.py <dir>/kt_kernel_trace.csv

Prints a markdown table, one row per case, and exits non-zero on a mismatch.  The cases run in table order and each
issues exactly one typed-aggregation launch (plus, for the twins' scene form, one agg_scene_kernel launch before it)."""
import csv
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
from launch_forms import FORWARD_CASES, case_forms  # noqa: E402

AGG = ("agg_x_kernel", "agg_mlp_kernel", "agg_rb2_kernel")


def main(path: str) -> int:
    with open(path) as fh:
        rows = sorted(csv.DictReader(fh), key=lambda r: int(r["Dispatch_Id"]))
    launches, scene = [], None
    for r in rows:
        grid = int(r["Grid_Size_X"]) // int(r["Workgroup_Size_X"])
        if "agg_scene_kernel" in r["Kernel_Name"]:
            scene = grid
            continue
        name = next((k for k in AGG if k in r["Kernel_Name"]), None)
        if name is not None:
            launches.append((name, grid, scene))
            scene = None
    if len(launches) != len(FORWARD_CASES):
        print(f"{len(launches)} aggregation launches in the trace, {len(FORWARD_CASES)} forward cases")
        return 2
    bad = 0
    print("| case | forms | kernel | expected grid | traced grid | scene form expected / traced | ok |")
    print("|---|---|---|---|---|---|---|")
    for c, (name, grid, scene) in zip(FORWARD_CASES, launches):
        f = case_forms(c)
        ok = name == f["agg_kernel"] and grid == f["agg_grid"] and scene == f["scene_grid"]
        bad += not ok
        forms = ", ".join(("node" if g["node_form"] else f"wpr{g['wpr']}") + (f"/spw{g['spw']}" if g["spw"] else "")
                          for g in f["groups"])
        print(f"| {c['id']} | {forms} | {name} | {f['agg_grid']} | {grid} | {f['scene_grid']} / {scene} | "
              f"{'yes' if ok else 'NO'} |")
    print(f"\n{len(launches) - bad}/{len(launches)} cases ran the expected form")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1]))
