#!/usr/bin/env python3
"""Entry point for the third training stage of the motion prior (`GAMMAPrimitiveComboTrainOP`,
motion/models/models_GAMMA_primitive.py:713-1093): the marker predictor fine-tuned through the frozen body regressor and SMPL-X.
The reference tree ships the operator and its config (`crowd_ppo/cfg_samp20/MPVAECombo_samp_2frame.yml`) but no script for
it; this one follows `train_GAMMARegressor.py`: `--cfg <name>` is looked up as `exp_GAMMAPrimitive/cfg/<name>.yml`, then
`crowd_ppo/cfg_samp20/<name>.yml`, under the working directory; results go to `results/exp_GAMMAPrimitive/<name>/`.

The combo yml names the predictor's and the regressor's configs (`modelconfig.predictor_config / regressor_config`); those two are
loaded the same way for their `modelconfig` and for the `save_dir` the pre-trained `epoch-300.ckp` / `epoch-100.ckp` are read
from (:759-770).  `--resume_training 1` continues from the newest checkpoint of the combo's own `save_dir` instead."""
import argparse
import os
import sys

import numpy as np
import torch
import yaml

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from egogen_amd.train_combo import GAMMAPrimitiveComboTrainOP  # noqa: E402
from egogen_amd.train_regressor import BatchGeneratorAMASSCanonicalized  # noqa: E402


def load_cfg(name, exp="exp_GAMMAPrimitive"):
    for f in (os.path.join(".", exp, "cfg", f"{name}.yml"), os.path.join(".", "crowd_ppo", "cfg_samp20", f"{name}.yml")):
        if os.path.exists(f):
            break
    else:
        raise FileNotFoundError(f"{name}.yml under ./{exp}/cfg or ./crowd_ppo/cfg_samp20")
    with open(f) as fh:
        cfg = yaml.safe_load(fh)
    exp_dir = os.path.join("results", exp, name)
    for sub in ("results", "checkpoints", "logs"):
        os.makedirs(os.path.join(exp_dir, sub), exist_ok=True)
    cfg.setdefault("trainconfig", {})
    cfg["trainconfig"]["save_dir"] = os.path.join(exp_dir, "checkpoints")
    cfg["trainconfig"]["log_dir"] = os.path.join(exp_dir, "logs")
    return cfg


def main(argv=None):
    parser = argparse.ArgumentParser()
    parser.add_argument("--cfg", default="MPVAECombo_samp_2frame")
    parser.add_argument("--resume_training", type=int, default=0)
    parser.add_argument("--verbose", type=int, default=1)
    parser.add_argument("--seed", type=int, default=0)
    parser.add_argument("--gpu_index", type=int, default=0)
    args = parser.parse_args(argv)
    np.random.seed(args.seed)
    torch.manual_seed(args.seed)
    cfg = load_cfg(args.cfg)
    predictorcfg = load_cfg(cfg["modelconfig"]["predictor_config"])
    regressorcfg = load_cfg(cfg["modelconfig"]["regressor_config"])
    losscfg, traincfg = cfg["lossconfig"], cfg["trainconfig"]
    traincfg["resume_training"] = args.resume_training == 1
    traincfg["verbose"] = args.verbose == 1
    traincfg["gpu_index"] = args.gpu_index
    trainop = GAMMAPrimitiveComboTrainOP(predictorcfg, regressorcfg, losscfg, traincfg)
    batch_gen = BatchGeneratorAMASSCanonicalized(amass_data_path=traincfg["dataset_path"], amass_subset_name=traincfg.get("subsets"),
                                                 sample_rate=int(traincfg.get("sample_rate", 3)),
                                                 body_repr=regressorcfg["modelconfig"]["body_repr"], read_to_ram=False)
    batch_gen.get_rec_list(shuffle_seed=args.seed)
    trainop.train(batch_gen)


if __name__ == "__main__":
    main()
