"""Routed feed-forward networks (reference: ``naive_gpt/layers/sparse/feedforward.py``).

The hidden dimension is cut into ``n_blocks = d_ff / block_size`` blocks; a sigmoid
router scores the blocks per token and only the top-k blocks are evaluated:
k = n_blocks // 2 for ``RoutedFFN`` (``feedforward.py:59-62``), n_blocks // 4 for
``RoutedLLaMaFFN`` (``:155-158``).  The plain variants do not weight the blocks by
the router probability (the LoRA variants in ``tuning/lora_ffn.py`` do).

Evaluation goes through ``routing.routed_apply``: tokens are bucketed per block
(every token appears in exactly k buckets) and each bucket runs a dense block
GEMM; see that module for the MI355X mapping.

bf16 layers (activations and every base weight bf16) take the grouped path on the bf16 kernels.
The router's Linear stays a torch bf16 op; its probabilities are widened to fp32 for the bucketing
(spt_route_topk), which ranks larger first and breaks exact ties towards the LOWER block index --
torch.topk leaves the order of ties unspecified, and bf16 probabilities tie far more often than
fp32 ones, so the loop and the grouped path may pick different blocks for a tied token.
"""
import torch
from torch import nn

from naive_gpt import ext, layers
from . import routing


def _make_router(d_model: int, n_blocks: int):
    return nn.Sequential(nn.Linear(d_model, n_blocks), nn.Sigmoid())


def _grouped_usable(x: torch.Tensor, *frozen) -> bool:
    from . import grouped
    if x.dtype == torch.bfloat16:
        return grouped.bf16_usable(x, *frozen)
    return grouped.usable(x, *frozen)


def _bf16_shapes_ok(x: torch.Tensor, d: int, bs: int) -> bool:
    from . import grouped
    return x.dtype != torch.bfloat16 or grouped.bf16_shapes(d, bs)


def _loop_why(x: torch.Tensor, trainable: bool, d: int, bs: int, *weights):
    """the fallback reason of the loop: a dtype mix, or bf16 shapes the bf16 kernels do not take, when
    that is what sends the layer there"""
    from . import grouped
    mix = grouped.dtype_mix(x, *weights)
    if mix:
        return mix
    if not _bf16_shapes_ok(x, d, bs):
        return 'bf16 d_model {} / block {}: multiples of 64 only'.format(d, bs)
    return 'x {} {}, trainable weights: {}'.format(tuple(x.shape), x.dtype, trainable)


def _combine(ys: torch.Tensor, bk, x: torch.Tensor) -> torch.Tensor:
    """y[t] = sum of the token's rows of ys, in block order (the reference's `y[mask] += ...` loop
    order): a fixed-order gather (spt_rows_combine, spt_rows_combine_bf16) where that applies."""
    if ys.is_cuda and ys.dtype == torch.float32 and ys.size(1) % 4 == 0 and not ys.requires_grad:
        return ext.rows_combine(ys.contiguous(), bk.pos)
    if ys.is_cuda and ys.dtype == torch.bfloat16 and ys.size(1) % 4 == 0 and not ys.requires_grad:
        return ext.rows_combine(ys.contiguous(), bk.pos)
    return torch.zeros_like(x).index_add_(0, bk.token_long, ys)


class RoutedFFN(layers.Feedforward):
    def __init__(self, d_model: int, d_feedforward: int, block_size: int,
                 activation: nn.Module, p_dropout: float = 0.0):
        super().__init__(d_model, d_feedforward, p_dropout=p_dropout,
                         activation=activation)
        self.block_size = block_size
        assert d_feedforward % block_size == 0
        self.n_blocks = d_feedforward // block_size
        self.router = _make_router(d_model, self.n_blocks)

    @staticmethod
    def from_pretrained(block_size: int, source: layers.Feedforward):
        assert isinstance(source, layers.Feedforward)
        model = RoutedFFN(block_size=block_size, d_model=source.d_model,
                          d_feedforward=source.d_feedforward,
                          activation=source.activation, p_dropout=source.p_dropout)
        report = model.load_state_dict(source.state_dict(), strict=False)
        if len(report.missing_keys) != 2:      # router weight + bias
            raise RuntimeError
        return model

    def _forward_grouped(self, x: torch.Tensor):
        """Frozen base weights on the GPU (a stage-'ffn'-only model, inference): the same device-side
        bucketing and grouped matrix-core GEMMs as the LoRA variant (layers/sparse/grouped.py), no
        host synchronisation -- the reference's loop reads every block's row count on the host
        (feedforward.py:66-85).  Trainable weights take _forward_trainable when
        grouped.TRAINABLE_WEIGHTS is on, the loop otherwise."""
        from . import grouped
        nb, bs, d = self.n_blocks, self.block_size, self.d_model
        prob = self.router(x)
        bk = grouped.make_buckets(prob.detach().float(), k=nb // 2)      # (bf16: widened for the bucketing)
        h = grouped.grouped_linear(x, self.fc1.weight, bk.offsets, (bs, d, bs * d, d, 1),
                                   gather=bk.token, gather_long=bk.token_long,
                                   bias=self.fc1.bias.view([nb, bs]))
        ys = grouped.grouped_linear(self.activation(h), self.fc2.weight, bk.offsets,
                                    (d, bs, bs, self.d_feedforward, 1))
        return _combine(ys, bk, x) + self.fc2.bias.view([1, -1])

    def _forward_trainable(self, x: torch.Tensor):
        """Trainable base weights on the grouped path (grouped.TRAINABLE_WEIGHTS): the same
        bucketing and block GEMMs, the weight gradients as grouped products over the bucket rows
        (grouped.RoutedFFNTrain).  The router only picks the blocks: no gradient reaches it."""
        from . import grouped
        prob = self.router(x)
        bk = grouped.make_buckets(prob.detach().float(), k=self.n_blocks // 2)
        if x.dtype == torch.bfloat16:
            return grouped.RoutedFFNTrainBf16.apply(x, self.fc1.weight, self.fc1.bias, self.fc2.weight,
                                                    self.fc2.bias, bk.token, bk.offsets, bk.pos, self.n_blocks,
                                                    grouped.activation_code(self.activation))
        return grouped.RoutedFFNTrain.apply(x, self.fc1.weight, self.fc1.bias, self.fc2.weight,
                                            self.fc2.bias, bk.token, bk.offsets, bk.pos, self.n_blocks,
                                            grouped.activation_code(self.activation))

    def _trainable_unusable(self, x: torch.Tensor):
        from . import grouped
        if not grouped.TRAINABLE_WEIGHTS:
            return None, False
        if self.d_model % 4 != 0 or self.block_size % 4 != 0:
            return 'd_model {} / block {}: multiples of 4 only'.format(self.d_model, self.block_size), True
        if not _bf16_shapes_ok(x, self.d_model, self.block_size):
            return 'bf16 d_model {} / block {}: multiples of 64 only'.format(self.d_model, self.block_size), True
        return grouped.trainable_unusable(x, grouped.activation_code(self.activation), self.fc1.weight,
                                          self.fc1.bias, self.fc2.weight, self.fc2.bias), True

    def forward(self, x: torch.Tensor):
        x_size = x.size()
        x = x.view([-1, self.d_model])
        bf16 = x.dtype == torch.bfloat16
        if _grouped_usable(x, self.fc1.weight, self.fc1.bias, self.fc2.weight, self.fc2.bias) \
                and self.d_model % 4 == 0 and self.block_size % 4 == 0 \
                and _bf16_shapes_ok(x, self.d_model, self.block_size):
            ext.note_path('routed_ffn_plain', 'grouped_bf16' if bf16 else 'grouped')
            return self._forward_grouped(x.contiguous()).view(x_size)
        why, on = self._trainable_unusable(x)
        if on and why is None:
            ext.note_path('routed_ffn_plain', 'grouped_trainable_bf16' if bf16 else 'grouped_trainable')
            return self._forward_trainable(x.contiguous()).view(x_size)
        if on:
            ext.note_path('routed_ffn_plain', 'torch_loop', fallback=x.is_cuda, why=lambda: why)
        else:
            ext.note_path('routed_ffn_plain', 'torch_loop', fallback=x.is_cuda,
                          why=lambda: _loop_why(x, self.fc1.weight.requires_grad, self.d_model, self.block_size,
                                                self.fc1.weight, self.fc1.bias, self.fc2.weight, self.fc2.bias))
        prob = self.router(x)
        route = routing.route_topk(prob, k=self.n_blocks // 2)
        w1 = self.fc1.weight.view([self.n_blocks, self.block_size, -1])
        b1 = self.fc1.bias.view([self.n_blocks, self.block_size])
        w2 = self.fc2.weight.view([-1, self.n_blocks, self.block_size])

        def block_fn(i, x_i, coeff_i):
            h = self.activation(torch.addmm(b1[i], x_i, w1[i].T))
            return torch.matmul(h, w2[:, i, :].T)

        y = routing.routed_apply(x, route, block_fn, weighted=False)
        y = y + self.fc2.bias.view([1, -1])
        return y.view(x_size)


class RoutedLLaMaFFN(layers.LLaMaFeedforward):
    def __init__(self, d_model: int, d_feedforward: int, block_size: int,
                 activation: nn.Module):
        super().__init__(d_model, d_feedforward, activation)
        self.block_size = block_size
        assert d_feedforward % block_size == 0
        self.n_blocks = d_feedforward // block_size
        self.router = _make_router(d_model, self.n_blocks)

    @staticmethod
    def from_pretrained(block_size: int, source: layers.LLaMaFeedforward):
        assert isinstance(source, layers.LLaMaFeedforward)
        model = RoutedLLaMaFFN(block_size=block_size, d_model=source.d_model,
                               d_feedforward=source.d_feedforward,
                               activation=source.activation)
        report = model.load_state_dict(source.state_dict(), strict=False)
        if len(report.missing_keys) != 2:
            raise RuntimeError
        return model

    def _forward_grouped(self, x: torch.Tensor):
        """see RoutedFFN._forward_grouped; top-k = n_blocks // 4 (feedforward.py:155-158)"""
        from . import grouped
        nb, bs, d = self.n_blocks, self.block_size, self.d_model
        prob = self.router(x)
        bk = grouped.make_buckets(prob.detach().float(), k=nb // 4)

        def up(linear):
            return grouped.grouped_linear(x, linear.weight, bk.offsets, (bs, d, bs * d, d, 1),
                                          gather=bk.token, gather_long=bk.token_long)

        h = self.activation(up(self.gate)) * up(self.side)
        ys = grouped.grouped_linear(h, self.down.weight, bk.offsets, (d, bs, bs, self.d_feedforward, 1))
        return _combine(ys, bk, x)

    def _forward_trainable(self, x: torch.Tensor):
        """see RoutedFFN._forward_trainable (grouped.RoutedLLaMAFFNTrain)"""
        from . import grouped
        prob = self.router(x)
        bk = grouped.make_buckets(prob.detach().float(), k=self.n_blocks // 4)
        if x.dtype == torch.bfloat16:
            return grouped.RoutedLLaMAFFNTrainBf16.apply(x, self.gate.weight, self.side.weight, self.down.weight,
                                                         bk.token, bk.offsets, bk.pos, self.n_blocks,
                                                         self.activation)
        return grouped.RoutedLLaMAFFNTrain.apply(x, self.gate.weight, self.side.weight, self.down.weight,
                                                 bk.token, bk.offsets, bk.pos, self.n_blocks, self.activation)

    def _trainable_unusable(self, x: torch.Tensor):
        from . import grouped
        if not grouped.TRAINABLE_WEIGHTS:
            return None, False
        if self.n_blocks < 4 or self.d_model % 4 != 0 or self.block_size % 4 != 0:
            return 'n_blocks {}, d_model {} / block {}: >= 4 blocks, multiples of 4 only'.format(
                self.n_blocks, self.d_model, self.block_size), True
        if not _bf16_shapes_ok(x, self.d_model, self.block_size):
            return 'bf16 d_model {} / block {}: multiples of 64 only'.format(self.d_model, self.block_size), True
        # (any activation: the gating product and its derivative are elementwise)
        return grouped.trainable_unusable(x, 0, self.gate.weight, self.side.weight, self.down.weight), True

    def forward(self, x: torch.Tensor):
        x_size = x.size()
        x = x.view([-1, self.d_model])
        bf16 = x.dtype == torch.bfloat16
        if self.n_blocks >= 4 and _grouped_usable(x, self.gate.weight, self.side.weight, self.down.weight) \
                and self.d_model % 4 == 0 and self.block_size % 4 == 0 \
                and _bf16_shapes_ok(x, self.d_model, self.block_size):
            ext.note_path('routed_ffn_plain', 'grouped_bf16' if bf16 else 'grouped')
            return self._forward_grouped(x.contiguous()).view(x_size)
        why, on = self._trainable_unusable(x)
        if on and why is None:
            ext.note_path('routed_ffn_plain', 'grouped_trainable_bf16' if bf16 else 'grouped_trainable')
            return self._forward_trainable(x.contiguous()).view(x_size)
        if on:
            ext.note_path('routed_ffn_plain', 'torch_loop', fallback=x.is_cuda, why=lambda: why)
        else:
            ext.note_path('routed_ffn_plain', 'torch_loop', fallback=x.is_cuda,
                          why=lambda: _loop_why(x, self.gate.weight.requires_grad, self.d_model, self.block_size,
                                                self.gate.weight, self.side.weight, self.down.weight))
        prob = self.router(x)
        route = routing.route_topk(prob, k=self.n_blocks // 4)
        gate = self.gate.weight.view([self.n_blocks, self.block_size, -1])
        side = self.side.weight.view([self.n_blocks, self.block_size, -1])
        down = self.down.weight.view([-1, self.n_blocks, self.block_size])

        def block_fn(i, x_i, coeff_i):
            h = self.activation(torch.matmul(x_i, gate[i].T)) * torch.matmul(x_i, side[i].T)
            return torch.matmul(h, down[:, i, :].T)

        y = routing.routed_apply(x, route, block_fn, weighted=False)
        return y.view(x_size)
