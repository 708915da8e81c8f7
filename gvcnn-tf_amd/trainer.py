"""Trainer parity layer: the host-side schedule around the training step.

    get_model_learning_rate(...)   utils/train_utils.py:65-118 ('step' = staircase exponential decay, 'poly' =
                                   polynomial decay to 0, slow start for the first steps)
    Trainer                        train.py:166-187,259-302: learning rate -> forward/backward/update (BN moving
                                   averages + Momentum) -> global step; `check_numerics` on the loss (train.py:175)

    Trainer.save / restore         tf.train.Saver's role (train.py:225-234,297-302): every variable of the engine (slim /
                                   Keras names), the Momentum slots (`<variable>/Momentum`, the slot name
                                   tf.train.MomentumOptimizer uses) and `global_step` as a TF checkpoint-v2 bundle
                                   (gvcnn-tf_amd/tf_checkpoint.py)

Pure host logic on top of gvcnn-tf_amd/training.py (no arithmetic on tensors here).  Not built: summaries.
"""
import math

import numpy as np


def get_model_learning_rate(learning_policy, base_learning_rate, learning_rate_decay_step,
                            learning_rate_decay_factor, training_number_of_steps, learning_power,
                            slow_start_step, slow_start_learning_rate, global_step):
    """utils/train_utils.py:65-118 evaluated for one `global_step` (the reference reads the TF global-step variable)."""
    if learning_policy == "step":
        # tf.train.exponential_decay(staircase=True)
        lr = base_learning_rate * learning_rate_decay_factor ** (global_step // learning_rate_decay_step)
    elif learning_policy == "poly":
        # tf.train.polynomial_decay(end_learning_rate=0, cycle=False)
        s = min(global_step, training_number_of_steps)
        lr = base_learning_rate * (1.0 - s / float(training_number_of_steps)) ** learning_power
    else:
        raise ValueError("Unknown learning policy.")
    return slow_start_learning_rate if global_step < slow_start_step else lr


class Trainer:
    """train.py's per-step protocol around a TrainGVCNN (or sharding.ShardedTrainGVCNN) engine.  Defaults are the
    reference's flag defaults (train.py:36-60)."""

    def __init__(self, engine, learning_policy="poly", base_learning_rate=0.001, learning_rate_decay_step=0.3,
                 learning_rate_decay_factor=1e-3, training_number_of_steps=300000, learning_power=0.9,
                 slow_start_step=0, slow_start_learning_rate=1e-4, momentum=0.9, weight_decay=None, check_every=1):
        self.engine = engine
        if weight_decay is None:        # the backbone's arg scope: inception_utils.py:30 (4e-5), resnet_utils.py:198 (1e-4)
            eng = getattr(engine, "eng", engine)
            weight_decay = 0.00004 if getattr(eng, "backbone", "") == "inception_v3" else 0.0001
        self.cfg = (learning_policy, base_learning_rate, learning_rate_decay_step, learning_rate_decay_factor,
                    training_number_of_steps, learning_power, slow_start_step, slow_start_learning_rate)
        self.momentum, self.weight_decay = momentum, weight_decay
        self.check_every = check_every
        self.global_step = 0

    def learning_rate(self):
        return get_model_learning_rate(*self.cfg, self.global_step)

    def step(self, views, labels):
        """One training step; returns the loss (device scalar).  Raises FloatingPointError like
        tf.debugging.check_numerics(total_loss, 'Loss is inf or nan.') (train.py:175) — the check reads the loss back,
        so `check_every` > 1 amortises that synchronisation."""
        loss = self.engine.train_step(views, labels, lr=self.learning_rate(), mu=self.momentum,
                                      weight_decay=self.weight_decay)
        self.global_step += 1
        if self.check_every and self.global_step % self.check_every == 0:
            v = float(loss.item())
            if math.isnan(v) or math.isinf(v):
                raise FloatingPointError("Loss is inf or nan.")
            # the group-assignment status word of THIS step, in the same synchronising readback: a score of exactly
            # 1.0 (bin == num_group) or NaN leaves a view in no group with a finite loss; the reference's host
            # group_scheme raises IndexError / ValueError there (nets/model.py:23, train.py:277)
            head = getattr(self._engine(), "head", None)          # (both engines have one; a stand-in without it has
            if head is not None:                                  # no assignment to check)
                head.check_status()
        return loss

    # -- checkpoints (tf.train.Saver: train.py:225-234 restores, train.py:297-302 saves) -------------------------------
    def _engine(self):
        return getattr(self.engine, "eng", self.engine)

    def state_dict(self):
        """{checkpoint key: ndarray}: the engine's variables under their slim / Keras names (trainable, BN moving
        statistics, the V scorer layers), the Momentum slots as `<variable>/Momentum`, and `global_step` (int64)."""
        eng = self._engine()
        out = {k: v.detach().cpu().numpy() for k, v in eng.params.items()}
        for k, v in eng.momentum.items():
            out[k + "/Momentum"] = v.detach().cpu().numpy()
        if hasattr(eng, "score_kernel"):
            from . import params as _params
            for i in range(eng.score_kernel.shape[0]):
                kn, bn = _params.scorer_names(eng.view_offset + i)
                out[kn] = eng.score_kernel[i].detach().cpu().numpy().reshape(-1, 1)
                out[bn] = eng.score_bias[i:i + 1].detach().cpu().numpy()
        out["global_step"] = np.asarray(self.global_step, dtype=np.int64)
        return out

    def save(self, prefix):
        """Writes `prefix.index` + `prefix.data-00000-of-00001` (checkpoint-v2)."""
        import os
        from . import tf_checkpoint
        tf_checkpoint.write_checkpoint(prefix, {k: np.ascontiguousarray(v) for k, v in self.state_dict().items()})
        # the `checkpoint` state file tf.train.Saver keeps next to its bundles (a text CheckpointState proto): what
        # tf.train.latest_checkpoint(--saved_checkpoint_dir) reads (train.py:225-234, eval.py:119-125)
        d, base = os.path.split(os.path.abspath(prefix))
        state = os.path.join(d, "checkpoint")
        older = []
        if os.path.exists(state):
            for line in open(state):
                if line.startswith("all_model_checkpoint_paths:"):
                    older.append(line.split(":", 1)[1].strip().strip('"'))
        paths = [p for p in older if p != base] + [base]
        with open(state, "w") as f:
            f.write('model_checkpoint_path: "%s"\n' % base)
            for p in paths:
                f.write('all_model_checkpoint_paths: "%s"\n' % p)

    @staticmethod
    def latest_checkpoint(checkpoint_dir):
        """tf.train.latest_checkpoint: the prefix named by `<dir>/checkpoint`, or None."""
        import os
        state = os.path.join(checkpoint_dir, "checkpoint")
        if not os.path.exists(state):
            return None
        for line in open(state):
            if line.startswith("model_checkpoint_path:"):
                p = line.split(":", 1)[1].strip().strip('"')
                p = p if os.path.isabs(p) else os.path.join(checkpoint_dir, p)
                return p if os.path.exists(p + ".index") else None
        return None

    def restore(self, prefix, strict=True):
        """Loads a checkpoint written by save() (or a TF-slim backbone checkpoint with strict=False: whatever names
        match are bound, e.g. ImageNet `InceptionV3/...` weights; the rest keeps its values).  Returns the names that
        were NOT found."""
        import torch
        from . import tf_checkpoint
        eng = self._engine()
        ck = tf_checkpoint.load_checkpoint(prefix)
        missing = []

        def bind(name, dst):
            if name not in ck:
                missing.append(name)
                return
            src = torch.as_tensor(np.asarray(ck[name])).reshape(dst.shape)
            dst.copy_(src.to(dst.dtype))
        for k, v in eng.params.items():
            bind(k, v)
        for k, v in eng.momentum.items():
            bind(k + "/Momentum", v)
        if hasattr(eng, "score_kernel"):
            from . import params as _params
            for i in range(eng.score_kernel.shape[0]):
                kn, bn = _params.scorer_names(eng.view_offset + i)
                bind(kn, eng.score_kernel[i])
                bind(bn, eng.score_bias[i:i + 1])
        if "global_step" in ck:
            self.global_step = int(np.asarray(ck["global_step"]).reshape(-1)[0])
        elif strict:
            missing.append("global_step")
        if strict and missing:
            raise KeyError("checkpoint %s lacks %d variables, e.g. %s" % (prefix, len(missing), missing[:3]))
        if hasattr(eng, "_packed_dirty"):
            eng._packed_dirty = True                      # the packed filter images are stale now
        return missing
