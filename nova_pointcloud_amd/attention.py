"""Cross-length training attention on MI355X: the reference's nn.MultiheadAttention(embed_dim, num_heads, batch_first=True)
calls of the point-cloud models (transformer_pointcloud_nova.py) and the EdgeAligner built on one.

EdgeAligner.forward (:192-223) ends in biattn(query = the current subset's edge features [B, n, E], key = value = the
concatenated edge features of the subsets generated so far [B, m, E]), m != n; AutoregressiveDiffusion._aggregate_features
(:256-274) calls another one (:236, :265-269) on all generated subsets at once. Both run inside
generate_pointcloud_autoregressive (:641-700), on the gradient path of training.

`MultiheadAttention` carries nn.MultiheadAttention's parameters under its names; its projections are torch GEMMs, its core
is `autograd.attention` (forward with the row log-sum-exp kept, backward on csrc/attn_bwd.hip, nothing of size Lq x Lk
stored in either pass) wherever `autograd.attention_supported` says so - bf16 on the GPU, head dimension 64 / 96, equal or
different query and key lengths - and F.scaled_dot_product_attention elsewhere (CPU, float32, dropout in training mode).
`EdgeAligner` is the reference's module assembled from neighbors.edge_features, that attention and point_embed.point_embed."""
import torch
import torch.nn.functional as F

from . import autograd, neighbors, point_embed


class MultiheadAttention(torch.nn.Module):
    """nn.MultiheadAttention(embed_dim, num_heads, dropout, bias, batch_first=True) with the same parameter names and shapes
    (in_proj_weight [3E, E], in_proj_bias [3E], out_proj.weight [E, E], out_proj.bias [E]) and the same initial values, so a
    state_dict moves between the two with strict=True. forward(query [B, Lq, E], key [B, Lk, E], value [B, Lk, E]) returns
    (out [B, Lq, E], None), as the reference unpacks it. No masks, no attention weights: need_weights=True raises, the
    [Lq, Lk] matrix is never formed."""

    def __init__(self, embed_dim, num_heads, dropout=0.0, bias=True):
        super().__init__()
        if embed_dim <= 0 or num_heads <= 0 or embed_dim % num_heads:
            raise ValueError(f"embed_dim must be a positive multiple of num_heads, got {embed_dim} and {num_heads}")
        self.embed_dim, self.num_heads, self.dropout = embed_dim, num_heads, float(dropout)
        self.head_dim = embed_dim // num_heads
        self.batch_first = True
        self.in_proj_weight = torch.nn.Parameter(torch.empty(3 * embed_dim, embed_dim))
        if bias:
            self.in_proj_bias = torch.nn.Parameter(torch.empty(3 * embed_dim))
        else:
            self.register_parameter("in_proj_bias", None)
        self.out_proj = torch.nn.Linear(embed_dim, embed_dim, bias=bias)
        self._reset_parameters()

    def _reset_parameters(self):  # nn.MultiheadAttention._reset_parameters
        torch.nn.init.xavier_uniform_(self.in_proj_weight)
        if self.in_proj_bias is not None:
            torch.nn.init.constant_(self.in_proj_bias, 0.0)
            torch.nn.init.constant_(self.out_proj.bias, 0.0)

    def forward(self, query, key, value, need_weights=False):
        if need_weights:
            raise ValueError("MultiheadAttention: need_weights=True would form the [Lq, Lk] attention matrix, which this module never does")
        E, h, d = self.embed_dim, self.num_heads, self.head_dim
        if query.dim() != 3 or key.dim() != 3 or value.dim() != 3 or query.shape[-1] != E or key.shape[-1] != E or value.shape[-1] != E:
            raise ValueError(f"MultiheadAttention: expected batch-first [B, L, {E}] tensors, got {tuple(query.shape)}, {tuple(key.shape)}, "
                             f"{tuple(value.shape)}")
        if key.shape[:2] != value.shape[:2] or key.shape[0] != query.shape[0]:
            raise ValueError(f"MultiheadAttention: key and value must share [B, Lk] and B with the query, got {tuple(query.shape)}, "
                             f"{tuple(key.shape)}, {tuple(value.shape)}")
        W, b = self.in_proj_weight, self.in_proj_bias
        part = lambda i: (W[i * E:(i + 1) * E], None if b is None else b[i * E:(i + 1) * E])
        B, Lq, Lk = query.shape[0], query.shape[1], key.shape[1]
        heads = lambda t, L: t.view(B, L, h, d).transpose(1, 2)
        q = heads(F.linear(query, *part(0)), Lq)
        k = heads(F.linear(key, *part(1)), Lk)
        v = heads(F.linear(value, *part(2)), Lk)
        p = self.dropout if self.training else 0.0
        if p == 0.0 and Lq > 0 and autograd.attention_supported(q, None, k):
            o = autograd.attention(q, k, v)
        else:
            o = F.scaled_dot_product_attention(q, k, v, dropout_p=p)
        return self.out_proj(o.transpose(1, 2).reshape(B, Lq, E)), None


class EdgeAligner(torch.nn.Module):
    """The reference's EdgeAligner (transformer_pointcloud_nova.py:155-223) under its own attribute and parameter names - biattn,
    edge_mlp.0 / edge_mlp.2 (present and unused in forward, as there), spatial_embed - so its entries of a reference checkpoint
    load with strict=True. forward(current_points [B, n, 3], current_features [B, n, E], neighbor_points, neighbor_features
    (lists of [B, m_i, 3] / [B, m_i, E])): edge features (centre minus the mean of the min(8, N) nearest neighbours' features,
    neighbors.edge_features) of the current subset and of every neighbour subset, the latter concatenated along the points
    (none: the current ones), attention of the current over them, plus spatial_embed(current_points) added by
    point_embed.point_embed in the kernel that forms it. Output [B, n, E] in the features' dtype. It runs on a GPU."""

    def __init__(self, embed_dim, num_heads=8):
        super().__init__()
        self.embed_dim, self.num_heads = embed_dim, num_heads
        self.biattn = MultiheadAttention(embed_dim, num_heads)
        self.edge_mlp = torch.nn.Sequential(torch.nn.Linear(embed_dim, embed_dim // 2), torch.nn.ReLU(),
                                            torch.nn.Linear(embed_dim // 2, embed_dim))
        self.spatial_embed = torch.nn.Linear(3, embed_dim)

    def extract_edge_features(self, points, features):
        return neighbors.edge_features(points, features, k=min(8, points.shape[1]))

    def forward(self, current_points, current_features, neighbor_points, neighbor_features):
        if len(neighbor_points) != len(neighbor_features):
            raise ValueError(f"EdgeAligner: {len(neighbor_points)} neighbour point sets but {len(neighbor_features)} feature sets")
        dtype = self.biattn.in_proj_weight.dtype
        current = self.extract_edge_features(current_points, current_features).to(dtype)
        others = [self.extract_edge_features(p, f).to(dtype) for p, f in zip(neighbor_points, neighbor_features)]
        everything = torch.cat(others, dim=1) if others else current
        aligned, _ = self.biattn(current, everything, everything)
        out = point_embed.point_embed(current_points, self.spatial_embed.weight, self.spatial_embed.bias, base=aligned)
        return out.to(current_features.dtype)
