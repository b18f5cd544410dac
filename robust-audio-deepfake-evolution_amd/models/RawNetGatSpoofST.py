"""RawGAT-ST (legacy plugin, the third member of the AASIST / RawNet2 family) on the radhip MI355X path.

Drop-in for the reference's models/RawNetGatSpoofST.py::Model(d_args): same constructor (the model_config dict),
same attribute names and registration order, hence the same state_dict keys, and
forward(x[B, 64600], Freq_aug) -> (proj_ST[B, 7], logits[B, 2]).

What runs where:
  front end   CONV.absmaxpool: the HIP kernel fusing the sinc conv (70 x 129 taps: first_conv 128 is made odd,
              reference :167-169), |.| and the 3x3 max-pool (csrc/sincconv.hip); the [B, 70, 64472] conv output is
              never written (reference :330-332). Both encoders read this one output
  encoders    encoder_T and encoder_S, six radhip.sinc.Residual_block each, on NHWC activations: the frozen-BN
              fused epilogues, the pooled-gradient path and the dead-bn1 handling apply as in AASIST
  graph head  three graph-attention layers. With RADHIP_GAT=1 the attention map and the aggregation of each are ONE
              launch of csrc/gat.hip forward and one backward (radhip.ops.GatAtt), the [B, N, N, D] pair tensor never
              reaches memory; by default (measured no faster at batch 24), on CPU tensors and in float64
              they are the module path (plain batched tensor ops). The projections, the node BatchNorm, SELU and the
              top-k pooling are torch

Reference semantics kept on purpose:
  * "T" is the branch whose nodes are the 23 spectral bins (max of |e| over time, dim 3, :338) and "S" the one whose
    nodes are the 29 time frames (max over dim 2, :344) - the names say the opposite;
  * softmax over dim -2 of the [B, N, N, 1] attention map (:73), i.e. over the neighbour index j; no temperature and
    no positional parameter;
  * GraphPool keeps max(int(N * k), 2) nodes (:126; AASIST's floor is 1) in descending-score order (torch.topk),
    after scaling every node by its sigmoid score (:131-132);
  * proj_T = Linear(14, 12) and proj_S = Linear(23, 12) (:319-320) hard-code the node counts 23 -> 14 and 29 -> 23
    of a 64 600-sample input; any other length fails there, as in the reference;
  * the ST graph is the elementwise product out_T * out_S [B, 32, 12] (:349), transposed to 12 nodes of 32.
"""
import os

import torch
import torch.nn as nn
import torch.nn.functional as F

from radhip import ops
from radhip.sinc import CONV, Residual_block


def gat_fused_enabled():
    """RADHIP_GAT=1 puts every eligible graph-attention layer on csrc/gat.hip. Off by default: at the conf's batch of
    24 the fused layer was not faster than the module path beyond the run-to-run spread (profiles/rawgat_bench.json,
    DESIGN 3.8)."""
    return os.environ.get("RADHIP_GAT", "0") != "0"


def attention_module_path(x, att_proj, att_weight):
    """The attention map and aggregation as batched tensor ops (reference :49-78): [B, N, D] -> [B, N, D].
    Any device, any floating dtype."""
    a = torch.tanh(att_proj(x.unsqueeze(2) * x.unsqueeze(1))) @ att_weight      # [B, N, N, 1]
    return F.softmax(a.squeeze(-1), dim=-1) @ x


class GraphAttentionLayer(nn.Module):
    """Reference models/RawNetGatSpoofST.py:10-94."""

    def __init__(self, in_dim, out_dim, **kwargs):
        super().__init__()
        self.att_proj = nn.Linear(in_dim, out_dim)
        self.att_weight = nn.Parameter(torch.empty(out_dim, 1))
        nn.init.xavier_normal_(self.att_weight)
        self.proj_with_att = nn.Linear(in_dim, out_dim)
        self.proj_without_att = nn.Linear(in_dim, out_dim)
        self.bn = nn.BatchNorm1d(out_dim)
        self.input_drop = nn.Dropout(p=0.2)
        self.act = nn.SELU(inplace=True)

    def forward(self, x):
        x = self.input_drop(x)
        if gat_fused_enabled() and ops.gat_eligible(x, self.att_proj, self.att_weight):
            agg, _ = ops.gat_att(x, self.att_proj, self.att_weight)
        else:
            agg = attention_module_path(x, self.att_proj, self.att_weight)
        x = self.proj_with_att(agg) + self.proj_without_att(x)
        B, N, D = x.shape
        return self.act(self.bn(x.reshape(B * N, D)).view(B, N, D))


class GraphPool(nn.Module):
    """Reference models/RawNetGatSpoofST.py:97-134."""

    def __init__(self, k, in_dim, p):
        super().__init__()
        self.k = k
        self.sigmoid = nn.Sigmoid()
        self.proj = nn.Linear(in_dim, 1)
        self.drop = nn.Dropout(p=p) if p > 0 else nn.Identity()
        self.in_dim = in_dim

    def forward(self, h):
        scores = self.sigmoid(self.proj(self.drop(h)))                   # [B, N, 1]
        n = max(int(h.size(1) * self.k), 2)
        _, idx = torch.topk(scores, n, dim=1)
        return torch.gather(h * scores, 1, idx.expand(-1, -1, h.size(2)))


def _encoder(filts):
    return nn.Sequential(
        nn.Sequential(Residual_block(nb_filts=filts[1], first=True)),
        nn.Sequential(Residual_block(nb_filts=filts[2])),
        nn.Sequential(Residual_block(nb_filts=filts[3])),
        nn.Sequential(Residual_block(nb_filts=filts[4])),
        nn.Sequential(Residual_block(nb_filts=filts[4])),
        nn.Sequential(Residual_block(nb_filts=filts[4])))


class Model(nn.Module):
    def __init__(self, d_args):
        super().__init__()
        self.d_args = d_args
        filts = d_args["filts"]
        self.conv_time = CONV(out_channels=filts[0], kernel_size=d_args["first_conv"], in_channels=1)
        self.first_bn = nn.BatchNorm2d(num_features=1)
        self.selu = nn.SELU(inplace=True)
        self.encoder_T = _encoder(filts)
        self.encoder_S = _encoder(filts)
        self.GAT_layer_T = GraphAttentionLayer(64, 32)
        self.GAT_layer_S = GraphAttentionLayer(64, 32)
        self.GAT_layer_ST = GraphAttentionLayer(32, 16)
        self.pool_T = GraphPool(0.64, 32, 0.3)
        self.pool_S = GraphPool(0.81, 32, 0.3)
        self.pool_ST = GraphPool(0.64, 16, 0.3)
        self.proj_T = nn.Linear(14, 12)
        self.proj_S = nn.Linear(23, 12)
        self.proj_ST = nn.Linear(16, 1)
        self.out_layer = nn.Linear(7, 2)

    def front(self, x, Freq_aug=False):
        """Front end shared by both encoders: x [B, L] -> [B, 1, 23, (L - 128) // 3], NHWC-strided (reference
        :328-335)."""
        if x.is_cuda:
            x = self.conv_time.absmaxpool(x.float(), mask=Freq_aug).unsqueeze(1)
        else:       # the CPU / float64 path: the raw conv, as the reference writes it
            x = F.max_pool2d(torch.abs(self.conv_time(x.unsqueeze(1), mask=Freq_aug).unsqueeze(1)), (3, 3))
        x = self.selu(self.first_bn(x))
        N, C, H, W = x.shape
        # C == 1: the NCHW bytes are already NHWC; restride so MIOpen picks its NHWC solvers
        return x.contiguous().as_strided((N, C, H, W), (C * H * W, 1, W * C, C))

    def forward(self, x, Freq_aug=False):
        x = self.front(x, Freq_aug)
        e_T = torch.abs(self.encoder_T(x)).max(dim=3)[0]                   # [B, C, 23]: max along time
        out_T = self.proj_T(self.pool_T(self.GAT_layer_T(e_T.transpose(1, 2))).transpose(1, 2))
        e_S = torch.abs(self.encoder_S(x)).max(dim=2)[0]                   # [B, C, 29]: max along frequency
        out_S = self.proj_S(self.pool_S(self.GAT_layer_S(e_S.transpose(1, 2))).transpose(1, 2))
        gat_ST = self.GAT_layer_ST((out_T * out_S).transpose(1, 2))        # 12 nodes of 32
        proj_ST = self.proj_ST(self.pool_ST(gat_ST)).flatten(1)
        return proj_ST, self.out_layer(proj_ST)
