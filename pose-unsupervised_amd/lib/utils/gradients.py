"""The gradient-norm watch (reference lib/utils/gradients.py), on the device.

``check_grad_norm`` compares the size of each loss's gradient with respect to the network's
per-view outputs.  The reference takes the row norms with torch ops and its caller reads one
scalar per loss back every step (function.py:434-457); here every loss costs one
``torch.autograd.grad`` and one posu_grad_row_norms launch, and the results stay on the device.
"""
from collections import OrderedDict

import torch

from posu import ops


def check_grad_norm(losses_dict, x, norm=1):
    """gradients.py:16-40: for each (name, loss) the sum over the views x of
    (sum of the per-sample norms of d loss / d view) / (samples with a non-zero norm), as a 0-dim
    float64 cuda tensor.  x: a tensor or a list of [N, ...] f32 cuda tensors of one shape; norm 1 or 2.
    A view the loss does not depend on is reported as the reference reports it and skipped; a loss
    that depends on no view raises ValueError (the reference fails with an AttributeError there)."""
    results = OrderedDict()
    if not isinstance(x, (list, tuple)):
        x = [x]
    for name, loss in losses_dict.items():
        grad_list = torch.autograd.grad(outputs=loss, inputs=list(x), grad_outputs=torch.ones_like(loss),
                                        create_graph=False, retain_graph=True, only_inputs=True, allow_unused=True)
        for idx, grad in enumerate(grad_list):
            if grad is None:
                print('grad of {} (view {}) is None'.format(name, idx))
        if all(g is None for g in grad_list):
            raise ValueError('check_grad_norm: loss %r has no gradient with respect to any view' % (name,))
        results[name] = ops.grad_row_norms(list(grad_list), norm)
    return results
