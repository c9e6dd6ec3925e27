"""``parameters(yaml_name)`` for the ostrack tracker (lib/test/parameter/ostrack.py:7-34): merge
``experiments/ostrack/<yaml_name>.yaml`` into the default config and fill the TrackerParams the tracker class reads."""
import os

from ..config import fresh_cfg, update_config_from_file
from ..evaluation.environment import env_settings
from ..params import TrackerParams

#: the ostrack family's own config tree, as the reference keeps one per family (lib/config/ostrack/config.py)
cfg = fresh_cfg()


def parameters(yaml_name: str, env=None):
    """`env`: an object with `prj_dir` / `save_dir` (the reference's `env_settings()` when this runs inside the reference tree --
    integration/lib/test/parameter/ostrack.py passes it); default: this repo's own settings."""
    params = TrackerParams()
    env = env_settings() if env is None else env
    update_config_from_file(os.path.join(env.prj_dir, "experiments/ostrack/%s.yaml" % yaml_name), cfg)
    params.cfg = cfg
    params.template_factor = cfg.TEST.TEMPLATE_FACTOR
    params.template_size = cfg.TEST.TEMPLATE_SIZE
    params.search_factor = cfg.TEST.SEARCH_FACTOR
    params.search_size = cfg.TEST.SEARCH_SIZE
    params.checkpoint = os.path.join(env.save_dir, "checkpoints/train/ostrack/%s/OSTrack_ep%04d.pth.tar" % (yaml_name, cfg.TEST.EPOCH))
    params.save_all_boxes = False
    #: candidate-elimination YAMLs: "masked" | "compact" (model_vitb.build_ostrack); None: the environment variable VB_CE_FORM, else "masked"
    params.ce_form = None
    #: "bf16" | "fp32", the fp32-equivalent mode of the patch-16 ViT models (model_vitb.build_ostrack); None: VB_PRECISION, else "bf16"
    params.precision = None
    return params
