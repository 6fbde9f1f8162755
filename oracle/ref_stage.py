"""Stage the reference's scripts under oracle/_ref/reference/ (called by __graft_entry__.build()).

tests/test_launcher.py runs the reference's own figure and table scripts UNCHANGED, in their own directory layout, through this
package's launcher.  Those scripts are the reference's program text and are never committed here; build() copies them from the
reference checkout (MCPC_REFERENCE_DIR, default oracle.gen_golden.REF, where the fixture generators read it) into oracle/_ref/,
which git ignores.  Only the Python sources are copied: no weights, figures or checkpoints.  Without a reference checkout nothing is staged and those tests skip with that reason.
"""
import os
import shutil

from oracle.gen_golden import REF

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STAGED = os.path.join(ROOT, "oracle", "_ref", "reference")
SCRIPTS = ("figure_2.py", "figure_3.py", "figure_4.py", "figure_5.py", "figure_6.py", "table_1.py")
PACKAGES = ("predictive_coding", "utils", "Deep_Latent_Gaussian_Models")


def reference_dir():
    return os.environ.get("MCPC_REFERENCE_DIR", REF)


def stage():
    """Copy the scripts and the packages they import; returns the staged directory, or None when there is no reference checkout."""
    src = reference_dir()
    if not all(os.path.isfile(os.path.join(src, s)) for s in SCRIPTS):
        return None
    if os.path.isdir(STAGED):
        shutil.rmtree(STAGED)
    os.makedirs(STAGED)
    for name in sorted(os.listdir(src)):
        if name.endswith(".py") and os.path.isfile(os.path.join(src, name)):
            shutil.copy2(os.path.join(src, name), os.path.join(STAGED, name))
    for pkg in PACKAGES:
        if os.path.isdir(os.path.join(src, pkg)):
            shutil.copytree(os.path.join(src, pkg), os.path.join(STAGED, pkg),
                            ignore=lambda d, names: [n for n in names if not (n.endswith(".py") or os.path.isdir(os.path.join(d, n)))
                                                     or n in ("__pycache__", "checkpoints")])
    for dirpath, _, _ in os.walk(STAGED):          # the copies are read-only in the reference; the tests and a rebuild need to remove them
        os.chmod(dirpath, 0o755)
    for dirpath, _, files in os.walk(STAGED):
        for f in files:
            os.chmod(os.path.join(dirpath, f), 0o644)
    return STAGED


if __name__ == "__main__":
    print(stage())
