"""torch.autograd glue for the external loss boundary (``ssnet_base.forward_logits`` / ``backward_logits``): the library's
forward and backward passes as one differentiable block, logits out, input gradient back."""
import torch


class UResNetFunction(torch.autograd.Function):
    """``logits = UResNetFunction.apply(net, sess, data)``: ``[N, *spatial, num_class]`` fp32 on the device, differentiable
    with respect to ``data``.

    The PARAMETER gradients do not appear in torch: the backward pass ADDS them to the net's flat gradient buffer, exactly
    like ``accum_gradients`` (read them with ``net.get_gradients()``, clear them with ``net.zero_gradients()``, step with
    ``net.apply_gradients()``); no torch ``.grad`` holds them.  Only ``data`` receives a torch gradient, and only when it
    requires one.  One forward may be pending per net: call ``backward()`` before the net runs anything else."""

    @staticmethod
    def forward(ctx, net, sess, data):
        ctx.net, ctx.sess = net, sess
        ctx.data_shape = tuple(data.shape) if isinstance(data, torch.Tensor) else None
        return net.forward_logits(sess, data.detach() if isinstance(data, torch.Tensor) else data)

    @staticmethod
    def backward(ctx, grad):
        want = bool(ctx.needs_input_grad[2])
        din = ctx.net.backward_logits(ctx.sess, grad, want_input_grad=want)
        if want and ctx.data_shape is not None:
            din = din.reshape(ctx.data_shape)
        return None, None, (din if want else None)
