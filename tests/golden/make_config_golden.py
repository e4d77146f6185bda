#!/usr/bin/env python3
"""Generate tests/golden/reference_configs.json from the reference's own YAML files (configs/*.yaml).

    python tests/golden/make_config_golden.py <reference tree>

Per file, only the keys `syntalker_amd.config` reads (which denoiser class and body-part widths a configuration selects, its
optimiser / schedule / RVQ-VAE settings), as YAML parses them.  tests/test_config.py writes them back out as YAML and loads
them through `config.load_args`, so that the test runs without the reference tree."""
import glob
import json
import os
import sys

import yaml

KEYS = ("model", "g_name", "trainer", "vqvae_type", "use_trans", "vqvae_latent_scale", "vqvae_squeeze_scale", "pose_rep", "pose_length",
        "lr_base", "lr_policy", "decay_epochs", "decay_rate", "warmup_epochs", "warmup_lr", "grad_norm", "opt", "opt_betas", "weight_decay")


def main(ref):
    out = {}
    for path in sorted(glob.glob(os.path.join(ref, "configs", "*.yaml"))):
        with open(path) as f:
            a = yaml.safe_load(f) or {}
        out[os.path.basename(path)] = {k: a[k] for k in KEYS if k in a}
    dst = os.path.join(os.path.dirname(os.path.abspath(__file__)), "reference_configs.json")
    with open(dst, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"wrote {dst}: {len(out)} configurations")


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])
