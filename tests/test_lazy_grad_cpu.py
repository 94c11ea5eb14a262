"""ops.LazyGrad, the link that carries a gradient beside autograd as a recipe: `file` on the consumer side, `take` on the producer side, driven with CPU tensors
through real autograd.  The producer here is y = 2 x; a consumer's loss is c <y, 1>, whose gradient of y it files as the recipe (c,) instead of the tensor
c 1.  Whatever route the recipes take, x.grad must come out as 2 (sum of c [+ the dense consumer's weight]).  No library, no device."""
import torch

from tcct_amd import ops

SHAPE = (2, 3, 4, 5)


class Producer(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, link, log):
        ctx.set_materialize_grads(False)
        ctx.link, ctx.log = link, log
        return 2 * x, x.view_as(x)

    @staticmethod
    def backward(ctx, dy, dalias):
        single, rest = ctx.link.take(dy)
        ctx.log.append((single, rest, dy))
        if single is not None:
            g = torch.full(SHAPE, float(single[1]))             # formed from the recipe: dy holds nothing
        else:
            g = torch.zeros(SHAPE) if dy is None else dy.clone()
            for _, c in rest:
                g = g + c
        return 2 * g + (0 if dalias is None else dalias), None, None


class Consumer(torch.autograd.Function):
    @staticmethod
    def forward(ctx, y, link, c):
        ctx.link, ctx.c, ctx.meta = link, c, (y.shape, y.dtype, y.device)
        return y.sum() * c

    @staticmethod
    def backward(ctx, g):
        return ctx.link.file((ctx.c * g.item(),), *ctx.meta), None, None


def _produce(link=None):
    x = torch.randn(SHAPE, requires_grad=True)
    link, log = link or ops.LazyGrad(), []
    y, alias = Producer.apply(x, link, log)
    return x, y, alias, link, log


def test_one_consumer_is_taken_as_the_single_recipe():
    x, y, _, link, log = _produce()
    Consumer.apply(y, link, 3.0).backward()
    (single, rest, dy), = log
    assert single is not None and single[1] == 3.0 and rest == []
    assert tuple(dy.shape) == SHAPE and dy.stride() == (0, 0, 0, 0) and dy.data_ptr() == single[0].data_ptr() and not dy.any()
    assert link.recipes == [] and ops.lazy_grads_pending(link) == 0
    assert torch.equal(x.grad, torch.full(SHAPE, 6.0))


def test_placeholder_added_to_a_dense_gradient_leaves_the_recipe_to_materialise():
    x, y, _, link, log = _produce()
    w = torch.randn(SHAPE)
    (Consumer.apply(y, link, 3.0) + (y * w).sum()).backward()
    (single, rest, dy), = log
    assert single is None and [r[1] for r in rest] == [3.0]
    assert dy.stride(0) != 0 and torch.equal(dy, w)             # dense, and without the consumer's part
    assert link.recipes == []
    assert torch.equal(x.grad, 2 * (w + 3.0))


def test_two_placeholders_added_to_each_other():
    x, y, _, link, log = _produce()
    (Consumer.apply(y, link, 3.0) + Consumer.apply(y, link, 0.5)).backward()
    (single, rest, dy), = log
    assert single is None and sorted(r[1] for r in rest) == [0.5, 3.0]
    assert not dy.any() and dy.data_ptr() not in [r[0].data_ptr() for r in rest]       # the sum of two placeholders: zeros of its own
    assert link.recipes == []
    assert torch.equal(x.grad, torch.full(SHAPE, 7.0))


def test_no_gradient_delivered_with_one_recipe_filed():
    link = ops.LazyGrad()
    ph = link.file((3.0,), SHAPE, torch.float32, 'cpu')
    assert ops.lazy_grads_pending(link) == 1 and tuple(ph.shape) == SHAPE
    single, rest = link.take(None)
    assert single is None and [r[1] for r in rest] == [3.0] and link.recipes == []


def test_nothing_filed():
    x, y, alias, link, log = _produce()
    w = torch.randn(SHAPE)
    (y * w).sum().backward()
    (single, rest, dy), = log
    assert single is None and rest == [] and torch.equal(dy, w)
    assert link.take(None) == (None, []) and link.take(torch.zeros(1).expand(SHAPE)) == (None, [])
    x2, y2, alias2, link2, log2 = _produce()
    alias2.sum().backward()                                     # only the alias used: dy is None and nothing is filed
    assert log2[0][0] is None and log2[0][1] == [] and log2[0][2] is None
    assert torch.equal(x2.grad, torch.ones(SHAPE))


def test_take_leaves_the_link_empty():
    link = ops.LazyGrad()
    ph = link.file((1.0,), SHAPE, torch.float32, 'cpu')
    link.file((2.0,), SHAPE, torch.float32, 'cpu')
    assert ops.lazy_grads_pending(link) == 2
    single, rest = link.take(ph)                                # two filed: not a single recipe, even though dy is the first one's placeholder
    assert single is None and len(rest) == 2
    assert link.recipes == [] and ops.lazy_grads_pending(link) == 0 and link.take(ph) == (None, [])


def test_placeholder_of_another_link_is_not_mistaken():
    xa, ya, _, la, loga = _produce()
    xb, yb, _, lb, logb = _produce()
    # consumer of ya files on lb by mistake of address (what a recycled address would do): ya's producer receives lb's placeholder while la holds its own recipe
    la.file((4.0,), SHAPE, torch.float32, 'cpu')
    Consumer.apply(ya, lb, 3.0).backward()
    (single, rest, dy), = loga
    assert single is None and [r[1] for r in rest] == [4.0]     # la's recipe is to be materialised; the foreign placeholder is just a (zero) dense gradient
    assert dy.stride(0) == 0 and dy.data_ptr() != rest[0][0].data_ptr()
    assert ops.lazy_grads_pending(la) == 0 and ops.lazy_grads_pending(lb) == 1
    assert torch.equal(xa.grad, torch.full(SHAPE, 8.0))


def test_registry_finds_the_link_by_address_until_the_step_resets_it():
    t = torch.zeros(SHAPE)
    link = ops.LazyGrad()
    ops.fpl_lazy_grad_reset()
    assert ops.LazyGrad.of(t) is None
    link.register(t)
    view = t.permute(0, 3, 1, 2).permute(0, 2, 3, 1)            # an NCHW view of a view, taken back: attributes are gone, the address is not
    assert ops.LazyGrad.of(view) is link
    link.file((1.0,), SHAPE, torch.float32, 'cpu')
    assert ops.lazy_grads_pending() == 1
    link.take(None)
    assert ops.lazy_grads_pending() == 0
    ops.fpl_lazy_grad_reset()
    assert ops.LazyGrad.of(t) is None
    link.register(t)
    del link                                                    # the producer's node owned it: with the node gone the entry is void, whatever sits at the address
    assert ops.LazyGrad.of(t) is None and ops.lazy_grads_pending() == 0
    ops.fpl_lazy_grad_reset()
