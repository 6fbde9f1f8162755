"""`python -m montecarlopredictivecoding_amd.run <script>`: the reference's scripts run UNCHANGED, in the reference's REAL layout.

VERDICT r4 (missing #1, #2): the reference's script directory holds regular packages `predictive_coding/` and `utils/`, and Python puts
that directory ahead of PYTHONPATH -- alias packages on PYTHONPATH lose; and most of the reference's call sites build their models on
the CPU (figure_2.py:29-75, figure_4.py:537, figure_5.py:25-27, figure_6.py:55-93).  The tests below lay out a script directory the way
/root/reference is laid out -- with DECOYS where the reference's own hot-path modules are (importing one raises) -- and run a
builder-written script shaped like figure_2.py / figure_6.py (models on the CPU) through the launcher."""
import json
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DECOY = "raise ImportError('decoy: the script directory\\'s own {} was imported instead of the engine-backed module')\n"


def lay_out_reference_shaped_directory(d):
    """predictive_coding/ and utils/ as REGULAR packages (like /root/reference): hot-path modules are decoys, utils.data / utils.plotting real."""
    d.mkdir(exist_ok=True)
    (d / "predictive_coding").mkdir()
    (d / "predictive_coding" / "__init__.py").write_text(DECOY.format("predictive_coding/__init__.py"))
    (d / "predictive_coding" / "pc_trainer.py").write_text(DECOY.format("predictive_coding/pc_trainer.py"))
    (d / "utils").mkdir()
    (d / "utils" / "__init__.py").write_text("")                                   # (the reference's is empty too)
    (d / "utils" / "model.py").write_text(DECOY.format("utils/model.py"))
    (d / "utils" / "training_evaluation.py").write_text(DECOY.format("utils/training_evaluation.py"))
    (d / "utils" / "plotting.py").write_text("def setup_fig(zero=False):\n    return 'the script\\'s own utils/plotting.py'\n")
    (d / "utils" / "data.py").write_text("MARK = 'the script\\'s own utils/data.py'\n")
    return d


def _env():
    env = dict(os.environ)
    env["PYTHONPATH"] = ROOT + (os.pathsep + env["PYTHONPATH"] if env.get("PYTHONPATH") else "")
    return env


def test_launcher_resolves_hot_path_imports_past_the_scripts_own_packages(tmp_path):
    d = lay_out_reference_shaped_directory(tmp_path)
    (d / "probe.py").write_text(
        "import sys, json\n"
        "import predictive_coding as pc\n"
        "import predictive_coding.pc_trainer as pt\n"
        "from predictive_coding.utils import slow_down_warning\n"
        "from utils.model import random_step, get_model, fe_fn\n"
        "from utils.training_evaluation import get_mcpc_trainer\n"
        "from utils.plotting import setup_fig\n"
        "import utils.data as ud\n"
        "import utils\n"
        "print(json.dumps(dict(pc=pc.PCTrainer.__module__, pt=pt.PCTrainer is pc.PCTrainer, rs=random_step.__module__,\n"
        "                      te=get_mcpc_trainer.__module__, fig=setup_fig(), data=ud.MARK, utils_file=utils.__file__,\n"
        "                      argv=sys.argv[1:], path0=sys.path[0], name=__name__, sdw=slow_down_warning.__module__)))\n")
    # started directly, the script hits the decoy (that IS the reference's layout problem) ...
    direct = subprocess.run([sys.executable, str(d / "probe.py")], capture_output=True, text=True, env=_env(), cwd=str(d), timeout=300)
    assert direct.returncode != 0 and "decoy" in direct.stderr
    # ... the alias PACKAGES of compat/ on PYTHONPATH alone would lose the same way (the script's directory comes first: VERDICT r4
    # missing #2; `-S` keeps the interpreter from importing compat/sitecustomize.py) ...
    env = _env()
    env["PYTHONPATH"] = os.path.join(ROOT, "compat") + os.pathsep + env["PYTHONPATH"]
    aliased = subprocess.run([sys.executable, "-S", str(d / "probe.py")], capture_output=True, text=True, env=env, cwd=str(d), timeout=300)
    assert aliased.returncode != 0 and "decoy" in aliased.stderr
    # ... which is why compat/ carries a sitecustomize.py: imported while the interpreter starts, BEFORE the script's directory is on
    # the path, it installs the launcher's finder -- `PYTHONPATH=<repo>/compat python figure_2.py` runs the script unchanged on the engine
    hooked = subprocess.run([sys.executable, str(d / "probe.py"), "--flag", "7"], capture_output=True, text=True, env=env, cwd=str(d), timeout=300)
    assert hooked.returncode == 0, hooked.stdout + hooked.stderr
    out = json.loads(hooked.stdout.strip().splitlines()[-1])
    assert out["pc"] == "montecarlopredictivecoding_amd.predictive_coding.pc_trainer" and out["rs"] == "montecarlopredictivecoding_amd.utils.model"
    assert out["fig"].startswith("the script") and out["data"].startswith("the script") and out["argv"] == ["--flag", "7"]
    assert os.path.samefile(out["path0"], str(d)) and out["name"] == "__main__"
    # through the launcher the four hot-path imports resolve to the engine-backed modules, everything else stays the script's own
    run = subprocess.run([sys.executable, "-m", "montecarlopredictivecoding_amd.run", str(d / "probe.py"), "--flag", "7"],
                         capture_output=True, text=True, env=_env(), cwd="/tmp", timeout=300)
    assert run.returncode == 0, run.stdout + run.stderr
    out = json.loads(run.stdout.strip().splitlines()[-1])
    assert out["pc"] == "montecarlopredictivecoding_amd.predictive_coding.pc_trainer" and out["pt"] is True
    assert out["rs"] == "montecarlopredictivecoding_amd.utils.model"
    assert out["te"] == "montecarlopredictivecoding_amd.utils.training_evaluation"
    assert out["sdw"] == "montecarlopredictivecoding_amd.predictive_coding.utils"
    assert out["fig"].startswith("the script") and out["data"].startswith("the script")
    assert os.path.samefile(out["utils_file"], str(d / "utils" / "__init__.py"))
    assert out["argv"] == ["--flag", "7"] and os.path.samefile(out["path0"], str(d)) and out["name"] == "__main__"


def test_launcher_without_any_utils_package_and_install_in_process(tmp_path):
    (tmp_path / "lonely.py").write_text("from utils.model import random_step\nimport predictive_coding as pc\nprint(random_step.__module__, pc.__name__)\n")
    run = subprocess.run([sys.executable, "-m", "montecarlopredictivecoding_amd.run", str(tmp_path / "lonely.py")],
                         capture_output=True, text=True, env=_env(), cwd=str(tmp_path), timeout=300)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout.split() == ["montecarlopredictivecoding_amd.utils.model", "montecarlopredictivecoding_amd.predictive_coding"]
    # install() inside a running interpreter (a notebook): same switch, idempotent, removable
    code = ("import sys; sys.path.insert(0, %r)\n"
            "import montecarlopredictivecoding_amd.run as r\n"
            "r.install(); r.install()\n"
            "assert sum(isinstance(f, r.EngineFinder) for f in sys.meta_path) == 1 and isinstance(sys.meta_path[0], r.EngineFinder)\n"
            "import predictive_coding as pc; assert pc.PCLayer.__module__.startswith('montecarlopredictivecoding_amd')\n"
            "r.uninstall(); assert not any(isinstance(f, r.EngineFinder) for f in sys.meta_path); print('ok')\n") % str(
        lay_out_reference_shaped_directory(tmp_path / "ref"))
    run = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=_env(), cwd="/tmp", timeout=300)
    assert run.returncode == 0 and run.stdout.strip() == "ok", run.stdout + run.stderr


@pytest.mark.gpu
@pytest.mark.parametrize("how", ["launcher", "pythonpath"])
def test_reference_layout_cpu_built_models_run_on_the_engine(tmp_path, how):
    """Done-criterion of VERDICT r4 next #1: decoy packages + a CPU-built model; `last_call_mode == "fused"`; the figure-2 posterior
    N(0.44, 0.2) and figure_6's |W0| law inside the bounds of tests/test_gpu_compat.py / tests/test_gpu_learning.py; x and param.grad
    back on the CPU."""
    d = lay_out_reference_shaped_directory(tmp_path)
    script = d / "figure_like.py"
    shutil.copy(os.path.join(ROOT, "tests", "compat_script", "cpu_built_models.py"), script)
    text = script.read_text()
    assert "montecarlopredictivecoding_amd" not in text.split('"""')[2] and ".cuda(" not in text.split('"""')[2] and "use_cuda" not in text.split('"""')[2]
    if how == "launcher":           # python -m montecarlopredictivecoding_amd.run figure_like.py
        cmd, env = [sys.executable, "-m", "montecarlopredictivecoding_amd.run", str(script)], _env()
    else:                           # PYTHONPATH=<repo>/compat python figure_like.py   (compat/sitecustomize.py installs the same finder)
        cmd, env = [sys.executable, str(script)], dict(os.environ, PYTHONPATH=os.path.join(ROOT, "compat"))
    run = subprocess.run(cmd, capture_output=True, text=True, env=env, cwd=str(d), timeout=900)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]
    out = json.loads([ln for ln in run.stdout.splitlines() if ln.startswith("{")][-1])
    assert out["trainer_module"] == "montecarlopredictivecoding_amd.predictive_coding.pc_trainer"
    assert out["random_step_module"] == "montecarlopredictivecoding_amd.utils.model" and out["setup_fig"].startswith("the script")
    assert "staged onto cuda" in run.stderr                                     # one RuntimeWarning per trainer says what happens
    f2, f6 = out["fig2"], out["fig6"]
    assert f2["mode"] == "fused" and f2["map_mode"] == "fused" and f2["x_device"] == "cpu"
    assert abs(f2["map"] - 0.44) < 2e-3
    assert abs(f2["mean"] - 0.44) < 0.02 and abs(f2["var"] - 0.2) < 0.02, f2      # bounds of tests/test_gpu_compat.py
    assert f6["mode"] == "fused" and f6["x_device"] == "cpu" and f6["grad_device"] == "cpu" and f6["param_device"] == "cpu"
    ref = np.load(os.path.join(ROOT, "tests", "golden", "g12_learning_reference_trajectories.npz"))["fig6_nv2_traj_mu_w"]
    ideal, rw = np.sqrt(2.0 * 5.0 / 2.0 - 1.0), np.abs(ref[-50:, 1]).mean()
    assert abs(f6["abs_w0"] - ideal) < max(0.05 * ideal, 2.0 * abs(rw - ideal)), (f6, rw)      # bounds of tests/test_gpu_learning.py
    assert abs(f6["abs_w0"] - rw) < 0.1 and abs(f6["mu_w0"] - 1.0) < 0.05, (f6, rw)


def test_off_path_names_come_from_the_scripts_own_module(tmp_path):
    """The reference's utils/training_evaluation.py also holds helpers its scripts import from the same module and that are NOT on the hot
    path (figure_2.py:17-19: kl_divergence_discrete, MNIST_LinearClassifier, train, test; figure_5.py:14: KLdivergence, get_paired_stat;
    table_1.py:8: get_fid).  They are not restated in this repository: a name the engine-backed module lacks is taken from the SCRIPT'S OWN
    module of that name -- executed with the finder active, so its own `import predictive_coding` / `from utils.model import` resolve to the
    engine -- while every hot-path name stays the engine's."""
    d = lay_out_reference_shaped_directory(tmp_path)
    (d / "utils" / "training_evaluation.py").write_text(
        "import numpy as np\n"
        "import predictive_coding as pc\n"                                      # like the reference's module (training_evaluation.py:12-13)
        "from utils.model import bernoulli_fn, fe_fn\n"
        "PC_SEEN = pc.PCTrainer.__module__\n"
        "def get_pc_trainer(*a, **k):\n    raise RuntimeError('the script\\'s own get_pc_trainer was called')\n"
        "def kl_divergence_discrete(p, q):\n    p = np.asarray(p, dtype=np.float64); q = np.asarray(q, dtype=np.float64)\n"
        "    return float(np.sum(np.where(p != 0, p * np.log(p / q), 0)))\n"
        "class MNIST_LinearClassifier:\n    OWNER = 'the script\\'s own utils/training_evaluation.py'\n")
    (d / "probe2.py").write_text(
        "import json\n"
        "from utils.training_evaluation import kl_divergence_discrete, MNIST_LinearClassifier\n"
        "from utils.training_evaluation import get_pc_trainer, get_mcpc_trainer, fe_fn\n"
        "import utils.training_evaluation as te\n"
        "try:\n    from utils.training_evaluation import no_such_name\n    missing = 'imported'\n"
        "except ImportError as e:\n    missing = 'ImportError'\n"
        "print(json.dumps(dict(kl=kl_divergence_discrete([0.5, 0.5], [0.25, 0.75]), cls=MNIST_LinearClassifier.OWNER,\n"
        "                      gpt=get_pc_trainer.__module__, fe=fe_fn.__module__, seen=te.PC_SEEN, missing=missing)))\n")
    run = subprocess.run([sys.executable, "-m", "montecarlopredictivecoding_amd.run", str(d / "probe2.py")],
                         capture_output=True, text=True, env=_env(), cwd=str(d), timeout=300)
    assert run.returncode == 0, run.stdout + run.stderr
    out = json.loads(run.stdout.strip().splitlines()[-1])
    assert abs(out["kl"] - (0.5 * np.log(2.0) + 0.5 * np.log(0.5 / 0.75))) < 1e-12 and out["cls"].startswith("the script")
    assert out["gpt"] == "montecarlopredictivecoding_amd.utils.training_evaluation"           # hot-path names stay the engine's
    assert out["fe"] == "montecarlopredictivecoding_amd.utils.model"
    assert out["seen"] == "montecarlopredictivecoding_amd.predictive_coding.pc_trainer"      # the own module's `import predictive_coding` -> engine
    assert out["missing"] == "ImportError"
    # the names every reference script imports from the two modules resolve one way or the other (engine-backed, or the fallback above)
    import re
    import montecarlopredictivecoding_amd.utils.model as um
    import montecarlopredictivecoding_amd.utils.training_evaluation as te
    wanted_model = {"sample_x_fn", "sample_x_fn_normal", "sample_x_fn_cte", "fe_fn", "bernoulli_fn", "fe_fn_mask", "zero_fn", "bernoulli_fn_mask",
                    "random_step", "get_model", "get_representations"}                         # /root/reference/utils/model.py:8-71
    assert all(hasattr(um, n) for n in wanted_model)
    engine_backed = {"get_pc_trainer", "get_mcpc_trainer", "get_mcpc_trainer_one_sample", "sample_pc", "get_mse_rec", "get_marginal_likelihood", "fe_fn"}
    assert all(n in vars(te) for n in engine_backed)


# the reference's scripts as build() stages them (oracle/ref_stage.py: copied from a reference checkout, never committed)
REFERENCE = os.path.join(ROOT, "oracle", "_ref", "reference")
NOT_STAGED = "the reference's scripts are not staged under oracle/_ref/ (build() stages them where a reference checkout is at hand)"


@pytest.mark.skipif(not os.path.isfile(os.path.join(REFERENCE, "figure_6.py")), reason=NOT_STAGED)
def test_the_references_own_figure_6_reaches_the_engine_unchanged():
    """The real thing, as far as a container without a GPU can take it: `/root/reference/figure_6.py`, UNCHANGED and in its own directory
    (next to the reference's predictive_coding/ and utils/ packages), started through the launcher.  Its import lines
    (figure_6.py:11-15: predictive_coding, utils.plotting, utils.model, utils.training_evaluation), its CPU-built model
    (figure_6.py:41-52) and its trainer factory must carry it to its first `train_on_batch` (figure_6.py:70) ON THIS PACKAGE'S TRAINER --
    where, without a HIP device, the call fails loudly (no CPU path); with one it is staged onto the GPU (tests/test_gpu_staging.py).
    Started directly, the same script runs the reference's own CPU loop: that difference is what the launcher is for."""
    if __import__("torch").cuda.is_available():
        pytest.skip("with a GPU the script would run its whole experiment (10 epochs x 25 batches x 40 noise levels)")
    for how in ("launcher", "pythonpath"):
        if how == "launcher":
            cmd, env = [sys.executable, "-m", "montecarlopredictivecoding_amd.run", os.path.join(REFERENCE, "figure_6.py")], _env()
        else:
            cmd, env = [sys.executable, os.path.join(REFERENCE, "figure_6.py")], dict(os.environ, PYTHONPATH=os.path.join(ROOT, "compat"))
        env["MPLBACKEND"] = "Agg"
        run = subprocess.run(cmd, capture_output=True, text=True, env=env, cwd="/tmp", timeout=600)
        assert run.returncode != 0
        err = run.stderr
        assert "MCPCLibraryError" in err and "no HIP device is visible" in err, err[-3000:]
        assert "figure_6.py\", line 70, in varying_langevin_noise" in err                      # its first train_on_batch
        assert os.path.join("montecarlopredictivecoding_amd", "predictive_coding", "pc_trainer.py") in err
        assert os.path.join(REFERENCE, "predictive_coding") not in err                         # the reference's own trainer was never entered


_SCRIPT_DRIVER = r'''
"""Written by tests/test_launcher.py: executes ONE of the reference's scripts, unchanged and in its own directory, with the engine finder
installed -- as `python -m montecarlopredictivecoding_amd.run <script>` does -- but under a module name other than `__main__`, so that its
imports and definitions run and its experiment driver (data sets, weeks of training) does not; then reports where its names came from
and, for the scripts that have one, calls the first experiment function that needs no data set."""
import importlib, json, os, runpy, sys, types

script, first_fn = sys.argv[1], (sys.argv[2] if len(sys.argv) > 2 else "")


def stand_in(name, **attrs):
    """An EMPTY module for a third-party package this image lacks (plots, videos, FID, MNIST download): nothing of the reference."""
    try:
        importlib.import_module(name)
        return
    except Exception:
        pass
    parts = name.split(".")
    for i in range(1, len(parts) + 1):
        sub = ".".join(parts[:i])
        if sub not in sys.modules:
            m = types.ModuleType(sub)
            m.__path__ = []
            sys.modules[sub] = m
            if i > 1:
                setattr(sys.modules[".".join(parts[:i - 1])], parts[i - 1], m)
    for k, v in attrs.items():
        setattr(sys.modules[name], k, v)


class _Unavailable:
    def __init__(self, *a, **k):
        raise RuntimeError("a stand-in of tests/test_launcher.py was called")


stand_in("seaborn")
stand_in("torchvision")
stand_in("torchvision.utils", save_image=_Unavailable)
stand_in("torchvision.datasets", MNIST=_Unavailable)
stand_in("torchvision.transforms", Compose=_Unavailable, ToTensor=_Unavailable, Normalize=_Unavailable, Lambda=_Unavailable)
stand_in("moviepy")
stand_in("moviepy.editor", VideoClip=_Unavailable)
stand_in("moviepy.video.io.bindings", mplfig_to_npimage=_Unavailable)
stand_in("pytorch_fid")

from montecarlopredictivecoding_amd import run
run.install()
sys.path.insert(0, os.path.dirname(script))
sys.argv = [script]
g = runpy.run_path(script, run_name="_reference_script_under_test")

ours = "montecarlopredictivecoding_amd."
report = {"origins": {}}
for name, obj in g.items():
    mod = getattr(obj, "__module__", None)
    if isinstance(mod, str) and (mod.startswith(ours) or mod.startswith("_mcpc_script_own") or mod in ("utils.data", "utils.plotting")):
        report["origins"][name] = mod
if "pc" in g:
    report["pc.PCTrainer"] = g["pc"].PCTrainer.__module__
    report["pc.PCLayer"] = g["pc"].PCLayer.__module__
report["modules"] = {k: getattr(sys.modules[k], "__name__", "?") for k in ("predictive_coding", "utils.model", "utils.training_evaluation") if k in sys.modules}
if first_fn:
    import tempfile
    try:
        g[first_fn](tempfile.mkdtemp())
        report["call"] = "returned"
    except Exception as exc:
        import traceback
        tb = traceback.extract_tb(exc.__traceback__)
        report["call"] = type(exc).__name__ + ": " + str(exc)[:300]
        report["frames"] = [(os.path.relpath(f.filename, "/"), f.name) for f in tb]
print("REPORT " + json.dumps(report))
'''

# script -> (names its import lines take from utils.model / utils.training_evaluation that must be ENGINE-backed, names that must come from
# the script's own utils/training_evaluation.py through run.script_own_attr, first experiment function that needs no data set)
_REFERENCE_SCRIPTS = {
    "figure_2.py": (["sample_x_fn_cte", "bernoulli_fn", "bernoulli_fn_mask", "fe_fn", "fe_fn_mask", "get_model", "get_representations", "random_step",
                     "get_pc_trainer", "get_mcpc_trainer"], ["kl_divergence_discrete", "MNIST_LinearClassifier", "train", "test"], "posterior_linear_model"),
    "figure_3.py": (["sample_x_fn", "zero_fn", "random_step", "get_model", "get_pc_trainer", "get_mcpc_trainer"], [], "generation_linear_model"),
    "figure_4.py": (["random_step", "get_model", "bernoulli_fn", "bernoulli_fn_mask", "fe_fn_mask", "sample_x_fn_normal", "sample_pc", "get_mcpc_trainer",
                     "get_pc_trainer", "fe_fn"], [], "mcpc_linear_learning"),
    "figure_5.py": (["bernoulli_fn", "zero_fn", "random_step", "get_model", "get_pc_trainer", "get_mcpc_trainer"], ["KLdivergence", "get_paired_stat"], ""),
    "table_1.py": (["get_model", "bernoulli_fn", "get_marginal_likelihood", "get_mse_rec"], ["get_fid"], ""),
}


@pytest.mark.skipif(not os.path.isfile(os.path.join(REFERENCE, "figure_2.py")), reason=NOT_STAGED)
@pytest.mark.parametrize("script", sorted(_REFERENCE_SCRIPTS))
def test_the_references_other_scripts_resolve_their_imports_and_reach_the_engine(script, tmp_path):
    """VERDICT r5 next #7.  `/root/reference/figure_2.py`, `figure_3.py`, `figure_4.py`, `figure_5.py` and `table_1.py`, UNCHANGED and in
    their own directory, with the engine finder installed (third-party packages the image lacks -- seaborn, torchvision, moviepy,
    pytorch_fid -- as EMPTY stand-in modules): every `from utils.model import ...` / `from utils.training_evaluation import ...` line
    resolves, hot-path names to this package, the others (figure_2.py:17-19 `train`, `test`, `MNIST_LinearClassifier`,
    `kl_divergence_discrete`; figure_5.py:14 `KLdivergence`, `get_paired_stat`; table_1.py:8 `get_fid`) to the reference's own
    utils/training_evaluation.py executed with the finder active; `utils.data` / `utils.plotting` stay the reference's.  Where a script
    has an experiment that needs no data set, its first `train_on_batch` is this package's -- which, without a HIP device, fails loudly
    (no CPU path).  Nothing of the reference is copied or shipped: it is executed where it lies."""
    if __import__("torch").cuda.is_available():
        pytest.skip("with a GPU the experiment functions would run for hours")
    engine_names, own_names, first_fn = _REFERENCE_SCRIPTS[script]
    driver = tmp_path / "driver.py"
    driver.write_text(_SCRIPT_DRIVER)
    env = _env()
    env["MPLBACKEND"] = "Agg"
    run = subprocess.run([sys.executable, str(driver), os.path.join(REFERENCE, script), first_fn], capture_output=True, text=True, env=env,
                         cwd=str(tmp_path), timeout=900)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]
    rep = json.loads([ln for ln in run.stdout.splitlines() if ln.startswith("REPORT ")][-1][7:])
    o = rep["origins"]
    for n in engine_names:
        assert o.get(n, "").startswith("montecarlopredictivecoding_amd."), (n, o.get(n))
    for n in own_names:
        assert o.get(n, "").startswith("_mcpc_script_own.utils.training_evaluation"), (n, o.get(n))
    assert rep["modules"].get("utils.model") == "montecarlopredictivecoding_amd.utils.model"
    assert rep["modules"].get("utils.training_evaluation") == "montecarlopredictivecoding_amd.utils.training_evaluation"
    if "pc.PCTrainer" in rep:
        assert rep["pc.PCTrainer"] == "montecarlopredictivecoding_amd.predictive_coding.pc_trainer"
        assert rep["pc.PCLayer"] == "montecarlopredictivecoding_amd.predictive_coding.pc_layer"
    for n in ("setup_fig", "get_mnist_data"):
        if n in o:
            assert o[n] in ("utils.plotting", "utils.data"), (n, o[n])                 # the reference's own, untouched
    if first_fn:
        assert rep["call"].startswith("MCPCLibraryError") and "no HIP device is visible" in rep["call"], rep["call"]
        files = [f for f, _ in rep["frames"]]
        assert any(f.endswith(os.path.join("montecarlopredictivecoding_amd", "predictive_coding", "pc_trainer.py")) for f in files)
        assert not any(f.startswith(os.path.join(REFERENCE.lstrip("/"), "predictive_coding")) for f in files)     # the reference's trainer was never entered
        assert any(name == first_fn for _, name in rep["frames"])


def test_alias_loader_leaves_the_engine_modules_identity_alone():
    """importing `predictive_coding` through the finder must not rename the real module (its __spec__ decides how relative
    imports inside it resolve and whether importlib.reload works)."""
    code = ("import warnings, importlib\n"
            "warnings.simplefilter('error', ImportWarning)\n"
            "from montecarlopredictivecoding_amd import run\nrun.install()\n"
            "import predictive_coding as pc, utils.model as um\n"
            "import montecarlopredictivecoding_amd.predictive_coding as real, montecarlopredictivecoding_amd.utils.model as rum\n"
            "assert pc is real and um is rum\n"
            "assert real.__spec__.name == real.__name__ == 'montecarlopredictivecoding_amd.predictive_coding', real.__spec__\n"
            "assert rum.__spec__.name == 'montecarlopredictivecoding_amd.utils.model' and rum.__package__ == 'montecarlopredictivecoding_amd.utils'\n"
            "from montecarlopredictivecoding_amd.utils.training_evaluation import get_pc_trainer      # (a relative import inside: no ImportWarning)\n"
            "importlib.reload(rum)\nprint('OK')\n")
    run = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=_env(), cwd="/tmp", timeout=300)
    assert run.returncode == 0 and run.stdout.strip().endswith("OK"), run.stdout + run.stderr
