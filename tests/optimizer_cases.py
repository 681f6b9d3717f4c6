"""Keras SGD, RMSprop and the InverseTimeDecay schedule [TF] restated in numpy, in the style of clip_cases.adam.

The arithmetic is the one include/gct2.h defines for gct2_optimizer_apply and gct2_loss_scale_begin_schedule, nothing measured: all
float32, every product, sum, quotient and root rounded once, in this order (g2 = the unscaled and clipped gradient, formed by
clip_cases.scaled and clip_cases.clip exactly as for gct2_adam_keras_clipped):
    SGD, momentum == 0:      p = p - lr * g2
    SGD, momentum > 0:       m = momentum * m - lr * g2;  p = p + m,  Nesterov: p = p + (momentum * m - lr * g2) with the new m
    RMSprop:                 v = rho * v + (1 - rho) * (g2 * g2)
             momentum == 0:  p = p - (lr * g2) / (sqrt(v) + epsilon)
             momentum > 0:   m = momentum * m + (lr * g2) / sqrt(v + epsilon);  p = p - m
    InverseTimeDecay:        q = float32(k) / decay_steps, floored when staircase;  lr = initial / (1 + decay_rate * q)
A slot a kind does not use comes back as it went in.  PARITY UNPINNED w.r.t. TensorFlow (there is none here): the formulas are those
of tf.keras optimizer_v2 (TF 2.4 - 2.6)."""
import numpy as np

import clip_cases as K

F = np.float32
SGD, RMSPROP = 1, 2                 # GCT2_OPT_SGD, GCT2_OPT_RMSPROP (tests compare them with the binding's constants)
WARMUP, INVERSE_TIME_DECAY = 0, 1   # GCT2_SCHEDULE_*

# (initial_learning_rate, decay_steps, decay_rate) of the two InverseTimeDecay schedules the reference keeps commented out (train.py:70, 73)
REFERENCE_SCHEDULES = ((2.0, 10_000, 1), (1e-5, 10_000, 1))
SCHEDULE_STEPS = (0, 1, 9_999, 10_000, 10_001, 123_456)


def sgd(p, m, g2, lr, momentum=0.0, nesterov=False):
    """(p, m) after one Keras SGD step on the (clipped) gradient g2; m is None (and stays None) for momentum == 0"""
    p, g2 = np.asarray(p, dtype=F), np.asarray(g2, dtype=F)
    lr, mom = F(lr), F(momentum)
    with np.errstate(all="ignore"):
        step = lr * g2
        if not momentum > 0:
            return p - step, m
        m = mom * np.asarray(m, dtype=F) - step
        if nesterov:
            return p + (mom * m - step), m
        return p + m, m


def rmsprop(p, m, v, g2, lr, rho=0.9, momentum=0.0, epsilon=1e-7):
    """(p, m, v) after one Keras RMSprop step on the (clipped) gradient g2; m is None (and stays None) for momentum == 0"""
    p, v, g2 = (np.asarray(a, dtype=F) for a in (p, v, g2))
    lr, rho, mom, eps = F(lr), F(rho), F(momentum), F(epsilon)
    with np.errstate(all="ignore"):
        v = rho * v + (F(1.0) - rho) * (g2 * g2)
        step = lr * g2
        if not momentum > 0:
            return p - step / (np.sqrt(v) + eps), m, v
        m = mom * np.asarray(m, dtype=F) + step / np.sqrt(v + eps)
        return p - m, m, v


def apply(kind, p, m, v, g, lr, hyper, mode=K.CLIP_NONE, threshold=0.0, ss=None, grad_mul=1.0, inv_scale=1.0):
    """one gct2_optimizer_apply over flat arrays: (p, m, v) with the slots the kind does not use returned unchanged"""
    g2 = K.clip(K.scaled(g, grad_mul, inv_scale), mode, threshold, ss)
    if kind == SGD:
        p2, m2 = sgd(p, m, g2, lr, hyper.get("momentum", 0.0), hyper.get("nesterov", False))
        return p2, m2, v
    return rmsprop(p, m, v, g2, lr, hyper.get("rho", 0.9), hyper.get("momentum", 0.0), hyper.get("epsilon", 1e-7))


def inverse_time_decay(k, initial, decay_steps, decay_rate, staircase=False):
    with np.errstate(all="ignore"):
        q = F(k) / F(decay_steps)
        if staircase:
            q = np.floor(q)
        return F(initial) / (F(1.0) + F(decay_rate) * q)
