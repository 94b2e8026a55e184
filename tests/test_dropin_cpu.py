"""The drop-in mechanics of SURVEY §8b (VERDICT r02 "missing" #1): `install_as_hulc2()` aliases LEAF modules only, so that
everything else `hulc2/training.py:20-25,40,51,95` imports from the reference's `hulc2` package (utils.utils, kl_callbacks,
the data modules, the rollout callbacks) still comes from the reference tree.

Each case runs in its own interpreter (sys.modules / sys.meta_path are process-wide state).  No GPU, no compute."""
import subprocess
import sys
import textwrap
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent

# every `_target_` under conf/model/** + conf/affordance/aff_detection/r3m.yaml this build implements
# (reference yaml:line -> class); the rest of conf/model/** (CLIP / ResNet encoders, BiLSTM, GCBC ...) stays the reference's own.
OURS = {
    "hulc2.models.hulc2.Hulc2": "conf/model/calvin_hulc++.yaml:14",
    "hulc2.models.perceptual_encoders.concat_encoders.ConcatEncoders": "conf/model/perceptual_encoder/gripper_cam.yaml:1",
    "hulc2.models.perceptual_encoders.vision_network.VisionNetwork": "conf/model/perceptual_encoder/rgb_static/default.yaml:1",
    "hulc2.models.perceptual_encoders.vision_network_gripper.VisionNetwork": "conf/model/perceptual_encoder/rgb_gripper/default.yaml:1",
    "hulc2.models.perceptual_encoders.vision_r3m.VisionR3M": "conf/model/perceptual_encoder/rgb_static/r3m.yaml:1",
    "hulc2.models.encoders.goal_encoders.VisualGoalEncoder": "conf/model/visual_goal/default.yaml:1",
    "hulc2.models.encoders.goal_encoders.LanguageGoalEncoder": "conf/model/language_goal/default.yaml:1",
    "hulc2.models.plan_encoders.plan_proposal_net.PlanProposalNetwork": "conf/model/plan_proposal/default.yaml:1",
    "hulc2.models.plan_encoders.plan_recognition_net.PlanRecognitionTransformersNetwork": "conf/model/plan_recognition/transformers.yaml:1",
    "hulc2.models.decoders.logistic_decoder_rnn.LogisticDecoderRNN": "conf/model/action_decoder/logistic_decoder_rnn_calvin.yaml:1",
    "hulc2.models.auxiliary_loss_networks.proj_vis_lang.ProjVisLang": "conf/model/proj_vis_lang/default.yaml:1",
    "hulc2.utils.distributions.Distribution": "conf/model/distribution/discrete.yaml:1",
    "hulc2.affordance.models.language_encoders.sbert_lang_encoder.SBertLang": "conf/model/language_encoder/sbert.yaml:1",
    "hulc2.affordance.pixel_aff_lang_detector.PixelAffLangDetector": "conf/affordance/aff_detection/r3m.yaml",
}

LOCATE = textwrap.dedent('''
    import importlib
    def locate(path):
        """hydra 1.1 `_locate`: longest importable module prefix, then getattr for the rest (hydra/_internal/utils.py)."""
        parts = path.split(".")
        for n in reversed(range(1, len(parts) + 1)):
            try:
                obj = importlib.import_module(".".join(parts[:n]))
            except Exception:
                if n == 1:
                    raise
                continue
            break
        for part in parts[n:]:
            obj = getattr(obj, part)
        return obj
''')


def run(*segments, paths=()):
    """each code segment is dedented on its own, then they run as one script in a fresh interpreter"""
    env_path = [str(p) for p in paths] + [str(ROOT)]
    code = "\n".join(textwrap.dedent(s) for s in segments)
    r = subprocess.run([sys.executable, "-c", LOCATE + code], capture_output=True, text=True, timeout=300,
                       env={"PYTHONPATH": ":".join(env_path), "PATH": "/usr/bin:/bin", "HOME": "/tmp"}, cwd="/tmp")
    assert r.returncode == 0, r.stdout + r.stderr
    return r.stdout


def make_tree(tmp_path):
    """a throw-away `hulc2/` with the shape of the reference's package: real packages, leaves on both sides of the alias line"""
    files = {
        "hulc2/__init__.py": "__project__ = 'throwaway'\n",
        "hulc2/utils/__init__.py": "",
        "hulc2/utils/utils.py": "def get_last_checkpoint(p):\n    return None\nWHO = 'reference'\n",
        "hulc2/utils/kl_callbacks.py": "class KLConstantSchedule:\n    WHO = 'reference'\n",
        "hulc2/utils/distributions.py": "class Distribution:\n    WHO = 'reference'\n",
        "hulc2/datasets/__init__.py": "",
        "hulc2/datasets/x.py": "from hulc2.utils.utils import WHO\nclass Hulc2SimdDataModule:\n    pass\n",
        # like the reference's hulc2/models/__init__.py:2-11 — imports a leaf that is aliased, at package import time
        "hulc2/models/__init__.py": "from hulc2.affordance.models.language_encoders.sbert_lang_encoder import SBertLang\n"
                                    "lang_encoders = {'sbert': SBertLang}\n",
        "hulc2/models/hulc2.py": "class Hulc2:\n    WHO = 'reference'\n",
        "hulc2/models/gcbc.py": "from hulc2.models.hulc2 import Hulc2\nclass GCBC(Hulc2):\n    pass\n",
        "hulc2/models/perceptual_encoders/__init__.py": "",
        "hulc2/models/perceptual_encoders/vision_clip.py": "class VisionClip:\n    WHO = 'reference'\n",
        "hulc2/models/perceptual_encoders/vision_network.py": "class VisionNetwork:\n    WHO = 'reference'\n",
        "hulc2/affordance/__init__.py": "",
        "hulc2/affordance/models/__init__.py": "",
        "hulc2/affordance/models/language_encoders/__init__.py": "",
        "hulc2/affordance/models/language_encoders/sbert_lang_encoder.py": "class SBertLang:\n    WHO = 'reference'\n",
        "hulc2/affordance/models/language_encoders/bert_lang_encoder.py": "class BERTLang:\n    WHO = 'reference'\n",
    }
    for rel, text in files.items():
        f = tmp_path / rel
        f.parent.mkdir(parents=True, exist_ok=True)
        f.write_text(text)
    return tmp_path


CHECK_TREE = '''
    import hulc2
    assert hulc2.__project__ == "throwaway"                       # the reference's own top package, not an alias
    import hulc2.utils.utils, hulc2.utils.kl_callbacks, hulc2.datasets.x, hulc2.models
    from hulc2.utils.utils import get_last_checkpoint, WHO
    assert WHO == "reference" and hulc2.utils.kl_callbacks.KLConstantSchedule.WHO == "reference"
    assert hulc2.datasets.x.Hulc2SimdDataModule.__module__ == "hulc2.datasets.x"
    import hulc2_amd.models.hulc2 as ours
    assert locate("hulc2.models.hulc2.Hulc2") is ours.Hulc2
    import hulc2.models.hulc2
    assert hulc2.models.hulc2 is ours                              # bound on its (reference) parent package
    assert locate("hulc2.utils.distributions.Distribution").__module__ == "hulc2_amd.utils.distributions"
    assert locate("hulc2.models.perceptual_encoders.vision_network.VisionNetwork").__module__.startswith("hulc2_amd.")
    assert locate("hulc2.models.perceptual_encoders.vision_clip.VisionClip").WHO == "reference"   # not built: stays the reference's
    assert locate("hulc2.affordance.models.language_encoders.bert_lang_encoder.BERTLang").WHO == "reference"
    # what the package re-exports from an aliased leaf is the MI355X class as well
    assert hulc2.models.SBertLang.__module__.startswith("hulc2_amd.") and hulc2.models.lang_encoders["sbert"] is hulc2.models.SBertLang
    # a reference module that subclasses an aliased class picks up the alias (training.py:44-49 "hack for gcbc" imports by module path)
    import hulc2.models.gcbc
    assert issubclass(hulc2.models.gcbc.GCBC, ours.Hulc2)
    assert ours.__spec__.name == "hulc2_amd.models.hulc2" and ours.__name__ == "hulc2_amd.models.hulc2"
    print("ok")
'''


def test_install_before_importing_the_reference_tree(tmp_path):
    tree = make_tree(tmp_path)
    out = run('''
        from hulc2_amd.compat import install_as_hulc2
        install_as_hulc2()
        install_as_hulc2()                                         # idempotent
    ''', CHECK_TREE, paths=[tree])
    assert out.strip().endswith("ok")


def test_install_after_the_reference_tree_was_imported(tmp_path):
    tree = make_tree(tmp_path)
    out = run('''
        import hulc2.models.hulc2, hulc2.utils.distributions, hulc2.utils.utils, hulc2.models
        assert hulc2.models.hulc2.Hulc2.WHO == "reference" and hulc2.models.SBertLang.WHO == "reference"
        from hulc2_amd.compat import install_as_hulc2
        install_as_hulc2()
    ''', CHECK_TREE, paths=[tree])
    assert out.strip().endswith("ok")


def test_every_implemented_target_resolves_without_any_reference_tree():
    """this image / the GPU box: no `hulc2` importable — parents are synthesised as empty packages"""
    out = run(f'''
        from hulc2_amd.compat import install_as_hulc2, uninstall_as_hulc2
        install_as_hulc2()
        for path in {sorted(OURS)!r}:
            cls = locate(path)
            assert cls.__module__.startswith("hulc2_amd."), (path, cls.__module__)
        import hulc2.models.hulc2 as m
        assert m.__name__ == "hulc2_amd.models.hulc2"
        try:
            import hulc2.utils.utils
        except ModuleNotFoundError:
            pass
        else:
            raise AssertionError("nothing should provide hulc2.utils.utils here")
        uninstall_as_hulc2()
        import sys
        assert not [k for k in sys.modules if k == "hulc2" or k.startswith("hulc2.")]
        print("ok")
    ''')
    assert out.strip().endswith("ok")


# third-party packages the reference imports that this image lacks: permissive stand-ins so that the reference's OWN modules can be
# imported here (names only — nothing of them is called).  Present packages (torch, numpy, transformers ...) are used as they are.
STUBS = '''
    import sys, types, importlib.machinery
    MISSING = ("git", "hydra", "omegaconf", "pytorch_lightning", "torchvision", "cv2", "pyhash", "wandb", "gym", "calvin_env", "r3m",
               "pytorch3d", "sentence_transformers", "segmentation_models_pytorch", "termcolor", "matplotlib", "plotly", "MulticoreTSNE",
               "lightning_lite", "sklearn_extra", "openai", "robot_io", "PIL", "pybullet", "quaternion", "numpy_quaternion", "ftfy", "kornia", "moviepy", "png", "skimage", "imageio", "tacto", "pyrender")
    class _Any:
        def __init__(self, *a, **k): pass
        def __call__(self, *a, **k):
            return a[0] if len(a) == 1 and callable(a[0]) and not k else _Any()       # usable as a decorator (factory)
        def __getattr__(self, k): return _Any()
        def __mro_entries__(self, bases): return (object,)
    class _Meta(type):
        def __getattr__(cls, k):
            if k.startswith("__"): raise AttributeError(k)
            return _Any()
    class _Stub(types.ModuleType):
        __path__ = []
        def __getattr__(self, k):
            if k.startswith("__"): raise AttributeError(k)
            v = _Meta(k, (), {"__init__": lambda self, *a, **kw: None, "__call__": lambda self, *a, **kw: (a[0] if len(a) == 1 and callable(a[0]) and not kw else _Any()),
                             "__getattr__": lambda self, n: _Any()}) if k[:1].isupper() else _Any()
            setattr(self, k, v)
            return v
    class _Finder:
        def find_spec(self, name, path=None, target=None):
            if name.split(".")[0] in MISSING:
                return importlib.machinery.ModuleSpec(name, self, is_package=True)
        def create_module(self, spec): return _Stub(spec.name)
        def exec_module(self, m): pass
    import hulc2_amd.compat                      # decides HAVE_HYDRA / HAVE_LIGHTNING before the stand-ins exist
    from transformers import (BertConfig, BertModel, BertTokenizer, DistilBertConfig, DistilBertModel,   # resolved (lazily, by transformers)
                              DistilBertTokenizer)                                                        # before a fake torchvision could confuse it
    sys.meta_path.append(_Finder())
'''


def make_reference_tree(tmp_path):
    """a `hulc2/` package laid out like the reference's at every module path the next test names: the entry point hulc2/training.py with
    its third-party imports (hydra, omegaconf, pytorch_lightning: served by the STUBS) and its hulc2.utils.utils import; hulc2/models/__init__.py
    importing aliased leaves at package import time; a reference model class subclassing an aliased one (gcbc); a reference-side leaf under
    every parent package of OURS, and the aliased leaves themselves as reference classes (the alias must win over them)"""
    files = {
        "hulc2/__init__.py": "",
        "hulc2/training.py": "import hydra\nfrom omegaconf import DictConfig, OmegaConf\nfrom pytorch_lightning import Callback, LightningModule, Trainer\n"
                             "from pytorch_lightning.strategies import DDPStrategy\n"
                             "from hulc2.utils.utils import get_git_commit_hash, get_last_checkpoint, initialize_pretrained_weights, print_system_env_info\n",
        "hulc2/utils/utils.py": "".join(f"def {f}(*a, **k):\n    return None\n" for f in ("get_git_commit_hash", "get_last_checkpoint",
                                                                                          "initialize_pretrained_weights", "print_system_env_info")),
        "hulc2/utils/kl_callbacks.py": "from pytorch_lightning import Callback\nclass KLConstantSchedule(Callback):\n    pass\n",
        "hulc2/utils/transforms.py": "import torch\nclass ScaleImageTensor:\n    pass\n",
        "hulc2/utils/tensor_utils.py": "import torch\n",
        "hulc2/utils/data_utils.py": "import numpy as np\n",
        "hulc2/datasets/hulc2_sim_data_module.py": "import pytorch_lightning as pl\nclass Hulc2SimdDataModule(pl.LightningDataModule):\n    pass\n",
        "hulc2/datasets/shm_dataset.py": "class ShmDataset:\n    pass\n",
        "hulc2/datasets/utils/shared_memory_loader.py": "from pytorch_lightning import Callback\nclass SignalCallback(Callback):\n    pass\n",
        "hulc2/rollout/rollout.py": "from pytorch_lightning import Callback\nclass Rollout(Callback):\n    pass\n",
        "hulc2/models/__init__.py": "from hulc2.affordance.models.language_encoders.bert_lang_encoder import BERTLang\n"
                                    "from hulc2.affordance.models.language_encoders.sbert_lang_encoder import SBertLang\n"
                                    "lang_encoders = {'bert': BERTLang, 'sbert': SBertLang}\n",
        "hulc2/models/gcbc.py": "from hulc2.models.hulc2 import Hulc2\nclass GCBC(Hulc2):\n    pass\n",
        "hulc2/models/encoders/language_network.py": "class SBert:\n    pass\n",
        "hulc2/models/decoders/deterministic_decoder.py": "class DeterministicDecoder:\n    pass\n",
        "hulc2/models/perceptual_encoders/proprio_encoder.py": "class IdentityEncoder:\n    pass\n",
        "hulc2/affordance/models/language_encoders/bert_lang_encoder.py": "class BERTLang:\n    pass\n",
    }
    for path in OURS:
        mod, _, cls = path.rpartition(".")
        files[mod.replace(".", "/") + ".py"] = f"class {cls}:\n    WHO = 'reference'\n"
    for rel, text in files.items():
        f = tmp_path / rel
        f.parent.mkdir(parents=True, exist_ok=True)
        f.write_text(text)
    for d in (tmp_path / "hulc2").rglob("*"):                      # every directory a package, as in the reference
        if d.is_dir() and not (d / "__init__.py").exists():
            (d / "__init__.py").write_text("")
    return tmp_path


@pytest.mark.parametrize("order", ["before", "after"])
def test_with_the_reference_tree_on_sys_path(order, tmp_path):
    """the imports of the reference's hulc2/training.py:20-25 and the `_target_`s Hydra instantiates at :40 / :95
    (conf/datamodule/calvin_default.yaml:6, conf/callbacks/kl_schedule/constant.yaml:1, conf/callbacks/rollout/default.yaml:3) still come
    from the reference; the model classes of conf/model/** come from this package.  The reference tree is the stand-in above, laid out as
    the reference's at every path named here."""
    tree = make_reference_tree(tmp_path)
    ref = f"{tree}/hulc2/"
    pre = "import hulc2.utils.distributions, hulc2.models.hulc2, hulc2.models\n" if order == "after" else ""
    code = f'''
        from hulc2_amd.compat import install_as_hulc2
        install_as_hulc2()
        import hulc2
        assert hulc2.__file__.startswith({ref!r})
        from hulc2.utils.utils import get_git_commit_hash, get_last_checkpoint, initialize_pretrained_weights, print_system_env_info
        assert get_last_checkpoint.__module__ == "hulc2.utils.utils"
        for path in ("hulc2.datasets.hulc2_sim_data_module.Hulc2SimdDataModule", "hulc2.utils.kl_callbacks.KLConstantSchedule",
                     "hulc2.rollout.rollout.Rollout", "hulc2.utils.transforms.ScaleImageTensor", "hulc2.datasets.shm_dataset.ShmDataset",
                     "hulc2.datasets.utils.shared_memory_loader.SignalCallback", "hulc2.utils.tensor_utils", "hulc2.utils.data_utils"):
            obj = locate(path)
            f = sys.modules[getattr(obj, "__module__", None) or obj.__name__].__file__
            assert f.startswith({ref!r}), (path, f)
        for path in {sorted(OURS)!r}:
            cls = locate(path)
            assert cls.__module__.startswith("hulc2_amd."), (path, cls.__module__)
        # unbuilt variants of conf/model/** keep resolving to the reference's classes
        for path in ("hulc2.models.plan_encoders.plan_recognition_net.PlanRecognitionTransformersNetwork",):
            assert locate(path).__module__.startswith("hulc2_amd.")
        for path in ("hulc2.models.encoders.language_network.SBert", "hulc2.models.decoders.deterministic_decoder.DeterministicDecoder",
                     "hulc2.models.perceptual_encoders.proprio_encoder.IdentityEncoder"):
            assert sys.modules[locate(path).__module__].__file__.startswith({ref!r}), path
        import hulc2.training                      # the entry point itself imports (its module-level imports = training.py:1-25)
        assert hulc2.training.__file__ == {ref + "training.py"!r}
        import hulc2.models.gcbc, hulc2_amd.models.hulc2
        assert issubclass(hulc2.models.gcbc.GCBC, hulc2_amd.models.hulc2.Hulc2)
        import hulc2.models
        assert hulc2.models.__file__.startswith({ref!r}) and hulc2.models.lang_encoders["sbert"].__module__.startswith("hulc2_amd.")
        print("ok")
    '''
    out = run(STUBS, pre, code, paths=[tree])
    assert out.strip().endswith("ok")
