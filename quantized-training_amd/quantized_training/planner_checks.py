"""What the fusion planners (fused.py, model_fusions.py, train_fusions.py, the QAT modules) ask of a module before a fused launch may
stand in for it: which hooks it carries, and which fake-quantizers quantize() has hung on it.  The four hook dicts of nn.Module are
named here, in quantize.py (which removes the hooks it registered) and in model_fusions._run_pre_hooks (which executes them) only.
A site that looks at another subset than its neighbours says so in a comment there."""
from .fake_quantize import FusedAmaxObsFakeQuantize
from .quantizer.quantizer import QScheme


def no_hooks(mod):
    """No hook of any kind: forward, forward-pre, backward, backward-pre."""
    return not (mod._forward_hooks or mod._forward_pre_hooks or mod._backward_hooks or mod._backward_pre_hooks)


def own_hook(fn):
    """Marks a hook the package itself registers (the context hooks model_fusions and train_fusions keep on an attention block)."""
    fn._qt_own_hook = True
    return fn


def no_foreign_hooks(mod):
    """No hook of any kind but the package's own (own_hook): nobody outside the package is handed the module's inputs or its result."""
    return all(getattr(h, "_qt_own_hook", False)
               for hooks in (mod._forward_hooks, mod._forward_pre_hooks, mod._backward_hooks, mod._backward_pre_hooks) for h in hooks.values())


def no_forward_hooks(mod):
    """No forward hook and no forward pre-hook (backward hooks not looked at): a fake-quantizer somebody hooked runs as the module it is."""
    return not (mod._forward_hooks or mod._forward_pre_hooks)


def no_output_hook(mod):
    """No forward hook (the other three dicts are not looked at): nobody is handed the module's result."""
    return not mod._forward_hooks


def only_pre_hooks(mod):
    """Forward pre-hooks at most (quantize()'s input fake-quantizers): no forward, backward or backward-pre hook."""
    return not (mod._forward_hooks or mod._backward_hooks or mod._backward_pre_hooks)


def hook_counts(mod, forward_pre=None, forward=None, backward_pre=None, backward=None):
    """Each hook dict given a count holds exactly that many hooks (a tuple: one of these counts); a dict left at None is not looked at."""
    for hooks, want in ((mod._forward_pre_hooks, forward_pre), (mod._forward_hooks, forward), (mod._backward_pre_hooks, backward_pre),
                        (mod._backward_hooks, backward)):
        if want is not None and (len(hooks) not in want if isinstance(want, tuple) else len(hooks) != want):
            return False
    return True


def quantize_hooks_only(mod, forward_pre=1, backward_pre=None):
    """Exactly the hooks quantize() registers for the module's holders: `forward_pre` forward pre-hooks and no forward hook; with
    `backward_pre` given also that many backward pre-hooks and no backward hook (else the backward dicts are not looked at)."""
    return hook_counts(mod, forward_pre, 0, backward_pre, None if backward_pre is None else 0)


def holder_fqs(mod, holder, *keys, exact=True):
    """The fake-quantizers mod.<holder>[key] in the order of `keys` when the holder exists and has EXACTLY these keys -- exact=False:
    CONTAINS them, it may have others -- else None.  `mod` may be None."""
    h = getattr(mod, holder, None)
    if h is None or (exact and len(h) != len(keys)) or any(k not in h for k in keys):
        return None
    return tuple(h[k] for k in keys)


def holder_fq(mod, holder, key="0", exact=False):
    """mod.<holder>[key] when the holder exists and contains the key -- exact: and no other key -- else None.  `mod` may be None."""
    h = getattr(mod, holder, None)
    return h[key] if h is not None and key in h and not (exact and len(h) != 1) else None


def linear_input_fq(linear):
    """The one input fake-quantizer (`activation_pre_process` = {"0"}) of a Linear reached through exactly one forward pre-hook (the other
    three dicts not looked at) -- or of a pt2e_fusion.PreparedLinear, where it is a graph node (`_qt_prepared`) -- else None."""
    if not (len(linear._forward_pre_hooks) == 1 or linear.__dict__.get("_qt_prepared")):
        return None
    return holder_fq(linear, "activation_pre_process", exact=True)


def plain_per_tensor(fq):
    """A FusedAmaxObsFakeQuantize that is not per-channel, has no outlier split, no histogram, neither MICROSCALING nor GROUP_WISE_AFFINE."""
    return (isinstance(fq, FusedAmaxObsFakeQuantize) and not fq.is_per_channel and fq.outlier_threshold is None and not fq.record_histogram
            and fq.qscheme not in (QScheme.MICROSCALING, QScheme.GROUP_WISE_AFFINE))
