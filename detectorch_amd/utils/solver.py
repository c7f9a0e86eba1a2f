"""The learning-rate schedule of the reference's training loop (lib/utils/solver.py, used at train_fast.py:125-127): steps with
decay and a warm-up, under the reference's names and signatures.  Plain Python; the values are the reference's Python floats
EXACTLY (tests/golden/solver_lr.npz), so the order of the operations is kept."""


def adjust_learning_rate(optimizer, lr):
    """Set the learning rate of every parameter group (solver.py:1-3).  With ClippedSGD(capturable=True) use its set_lr_ instead,
    which also rewrites the device copy the kernels read."""
    for param_group in optimizer.param_groups:
        param_group['lr'] = lr


def get_step_index(cur_iter, lr_steps=[0, 240000, 320000], max_iter=360000):
    """The index of the learning-rate step iteration cur_iter is in (solver.py:6-13): the last step that has begun; from max_iter
    on, the number of steps."""
    if lr_steps[0] != 0:
        raise AssertionError('the first learning-rate step starts at iteration 0')
    bounds = list(lr_steps) + [max_iter]
    begun = [k for k, step in enumerate(bounds) if cur_iter < step]
    return (begun[0] if begun else len(bounds) - 1) - 1


def lr_func_steps_with_decay(cur_iter, base_lr=0.01, gamma=0.1):
    """lr = base_lr * gamma ** step index (solver.py:16-30)."""
    return base_lr * gamma ** get_step_index(cur_iter)


def get_lr_at_iter(it, warm_up_iters=500, warm_up_factor=0.3333333333333333, warm_up_method='linear'):
    """The learning rate of iteration `it` (solver.py:32-44): the stepped rate, during the first warm_up_iters iterations times a
    factor that is constant or rises linearly from warm_up_factor to 1.  KeyError on another warm_up_method, raised only while
    warming up, as in the reference."""
    lr = lr_func_steps_with_decay(it)
    if it >= warm_up_iters:
        return lr
    if warm_up_method == 'linear':
        alpha = it / warm_up_iters
        factor = warm_up_factor * (1 - alpha) + alpha
    elif warm_up_method == 'constant':
        factor = warm_up_factor
    else:
        raise KeyError('unknown warm_up_method %r' % (warm_up_method,))
    return lr * factor
