"""Restatement of the LoRA merge for the tests (CPU, torch only; nothing of adaface_amd is imported).

  merge:   W' = W + sum_a s_a * up_a @ down_a, in fp64 (merge64) and in fp32 in the kernel's order of additions (merge32);
  layout:  element (o, c, tap) of a weight [rows][cin][kk] lies at  (row_off + perm(o)) * ldw + tap * cin_pad + c  of the packed
           buffer, perm the GEGLU row order (value / gate groups of 16 interleaved), columns cin <= c < cin_pad zero;
  bound:   per element |got - ref64| <= (R_total + A + 2) * 2^-24 * (|W| + sum_a |s_a| * sum_r |up| |down|) + one unit in the last
           place of the storage type at |ref| (no second term for f32).  The first term is the classic bound of an fp32 dot product
           of R_total products followed by A scaled additions (each operation at most 2^-24 relative, first order, with 2 to spare
           for the final additions' own roundings); the second is the single rounding to storage, a full unit because the fp32
           error can flip a tie;
  names:   the kohya keys of a U-Net / text tower generated from the constructor arguments by diffusers' block structure, with
           the ldm name each must map onto, by the index formulas of the feature's description.
"""
import torch

STORAGE = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
MANT_BITS = {"f32": 23, "bf16": 7, "f16": 10}


# ---------------------------------------------------------------------------------------------------------------- merge
def _flat(base, up, down):
    rows = base.shape[0]
    r = down.shape[0]
    return base.reshape(rows, -1), up.reshape(rows, r), down.reshape(r, -1)


def merge64(base, adapters):
    """fp64 [rows, cin * kk] (the weight's own flat order, c * kk + tap)"""
    w = base.reshape(base.shape[0], -1).double().clone()
    for up, down, s in adapters:
        _, u, d = _flat(base, up, down)
        w += float(torch.tensor(s, dtype=torch.float32)) * (u.double() @ d.double())
    return w


def merge32(base, adapters):
    """fp32, adapters added one after the other as the kernel does: exact for exact-operand adapters but for the additions"""
    w = base.reshape(base.shape[0], -1).float().clone()
    for up, down, s in adapters:
        _, u, d = _flat(base, up, down)
        acc = (u.double() @ d.double())                       # (exact for the integer operands of the exact tests)
        term = (torch.tensor(s, dtype=torch.float32).double() * acc)
        assert torch.equal(term.float().double(), term), "merge32 is for exact-operand adapters"
        w = (w.double() + term).float()                       # one fp32 rounding per adapter
    return w


def magnitude(base, adapters):
    m = base.reshape(base.shape[0], -1).double().abs()
    for up, down, s in adapters:
        _, u, d = _flat(base, up, down)
        m = m + abs(float(torch.tensor(s, dtype=torch.float32))) * (u.double().abs() @ d.double().abs())
    return m


def ulp(ref, dtype):
    """one unit in the last place of the storage type at |ref| (fp64)"""
    lo = 2.0 ** -14 if dtype == "f16" else 2.0 ** -126
    e = torch.floor(torch.log2(ref.abs().clamp_min(lo)))
    return torch.pow(torch.tensor(2.0, dtype=torch.float64), e - MANT_BITS[dtype])


def bound(base, adapters, dtype):
    ref = merge64(base, adapters)
    n_ops = sum(int(d.shape[0]) for _, d, _ in adapters) + len(adapters) + 2
    b = n_ops * 2.0 ** -24 * magnitude(base, adapters)
    return ref, (b if dtype == "f32" else b + ulp(ref, dtype))


# ---------------------------------------------------------------------------------------------------------------- layout
def geglu_perm(n, half):
    j = n if n < half else n - half
    return (j >> 4) * 32 + (0 if n < half else 16) + (j & 15)


def packed_index(o, c, tap, rows, cin_pad, ldw, row_off=0, perm=False):
    rr = geglu_perm(o, rows // 2) if perm else o
    return (row_off + rr) * ldw + tap * cin_pad + c


def pack(flat, cin, kk, cin_pad=None, ldw=None, row_off=0, rows_total=None, perm=False, fill=0.0):
    """flat [rows, cin * kk] (column c * kk + tap) -> the packed [rows_total, ldw] buffer (same dtype); what the layout does not
    own holds `fill`, the padding columns zero."""
    rows = flat.shape[0]
    cin_pad = cin if cin_pad is None else cin_pad
    ldw = kk * cin_pad if ldw is None else ldw
    rows_total = row_off + rows if rows_total is None else rows_total
    out = torch.full((rows_total * ldw,), fill, dtype=flat.dtype)
    o = torch.arange(rows)
    half = rows // 2
    if perm:
        j = torch.where(o < half, o, o - half)
        rr = (j // 16) * 32 + torch.where(o < half, 0, 16) + (j % 16)
    else:
        rr = o
    cp, tap = torch.arange(cin_pad), torch.arange(kk)
    idx = ((row_off + rr)[:, None, None] * ldw + tap[None, :, None] * cin_pad + cp[None, None, :])      # [rows, kk, cin_pad]
    vals = torch.zeros(rows, kk, cin_pad, dtype=flat.dtype)
    vals[:, :, :cin] = flat.reshape(rows, cin, kk).permute(0, 2, 1)
    out[idx.reshape(-1)] = vals.reshape(-1)
    return out.reshape(rows_total, ldw)


# ---------------------------------------------------------------------------------------------------------------- state dicts
def merged_state_dict(sd, adapter_list, prefix="", exact=False):
    """sd with every touched '<prefix><name>.weight' replaced by its merge; adapter_list = [(weights, scale)], weights =
    {name: (up, down, alpha)}.  exact: merge32 (the fused load's bits for exact operands), else fp64 rounded to fp32."""
    out = dict(sd)
    names = sorted({n for w, _ in adapter_list for n in w})
    for n in names:
        key = prefix + n + ".weight"
        base = sd[key]
        ads = [(w[n][0], w[n][1], scale * float(w[n][2]) / w[n][1].shape[0]) for w, scale in adapter_list if n in w]
        flat = merge32(base, ads) if exact else merge64(base, ads).float()
        out[key] = flat.reshape(base.shape)
    return out


def exact_adapter(shapes, names, rank, seed, alpha_shift=8):
    """{name: (up, down, alpha)} with integer entries in [-4, 4] and alpha = rank * 2^-alpha_shift: s = scale * 2^-alpha_shift"""
    g = torch.Generator().manual_seed(seed)
    out = {}
    for n in names:
        shp = shapes[n]
        up = torch.randint(-4, 5, (shp[0], rank) + (1,) * (len(shp) - 2), generator=g).float()
        down = torch.randint(-4, 5, (rank,) + tuple(shp[1:]), generator=g).float()
        out[n] = (up, down, rank * 2.0 ** -alpha_shift)
    return out


def random_adapter(sd, prefix, names, rank, seed, ratio=1.0 / 3.0):
    """normal operands, alpha chosen so that rms(s * up @ down) = ratio * rms(W) at scale 1"""
    g = torch.Generator().manual_seed(seed)
    out = {}
    for n in names:
        w = sd[prefix + n + ".weight"]
        shp = w.shape
        up = torch.randn((shp[0], rank) + (1,) * (len(shp) - 2), generator=g)
        down = torch.randn((rank,) + tuple(shp[1:]), generator=g)
        delta = up.reshape(shp[0], rank).double() @ down.reshape(rank, -1).double()
        s = ratio * float(w.double().pow(2).mean().sqrt()) / float(delta.pow(2).mean().sqrt())
        out[n] = (up, down, s * rank)
    return out


# ---------------------------------------------------------------------------------------------------------------- names
def kohya_unet_names(cfg):
    """[(kohya module name behind 'lora_unet_', ldm parameter name without '.weight')] of every conv / linear layer diffusers'
    UNet2DConditionModel has for this config (cfg: channel_mult, num_res_blocks, attention_resolutions, transformer_depth)."""
    n, mult = cfg.num_res_blocks, list(cfg.channel_mult)
    nlev = len(mult)
    out = [("conv_in", "input_blocks.0.0"), ("conv_out", "out.2"), ("time_embedding_linear_1", "time_embed.0"),
           ("time_embedding_linear_2", "time_embed.2")]

    def resnet(k, p, shortcut):
        out.extend([(k + "_conv1", p + ".in_layers.2"), (k + "_conv2", p + ".out_layers.3"), (k + "_time_emb_proj", p + ".emb_layers.1")])
        if shortcut:
            out.append((k + "_conv_shortcut", p + ".skip_connection"))

    def attention(k, p):
        out.extend([(k + "_proj_in", p + ".proj_in"), (k + "_proj_out", p + ".proj_out")])
        for d in range(cfg.transformer_depth):
            kt, pt = f"{k}_transformer_blocks_{d}", f"{p}.transformer_blocks.{d}"
            for a in ("attn1", "attn2"):
                out.extend([(f"{kt}_{a}_to_{x}", f"{pt}.{a}.to_{x}") for x in "qkv"])
                out.append((f"{kt}_{a}_to_out_0", f"{pt}.{a}.to_out.0"))
            out.extend([(kt + "_ff_net_0_proj", pt + ".ff.net.0.proj"), (kt + "_ff_net_2", pt + ".ff.net.2")])

    ch, ds, skips = 1, 1, [1]
    for i in range(nlev):                                        # down blocks
        has_attn = ds in cfg.attention_resolutions
        for j in range(n):
            b = 1 + (n + 1) * i + j
            resnet(f"down_blocks_{i}_resnets_{j}", f"input_blocks.{b}.0", ch != mult[i])
            ch = mult[i]
            skips.append(ch)
            if has_attn:
                attention(f"down_blocks_{i}_attentions_{j}", f"input_blocks.{b}.1")
        if i != nlev - 1:
            out.append((f"down_blocks_{i}_downsamplers_0_conv", f"input_blocks.{(n + 1) * (i + 1)}.0.op"))
            skips.append(ch)
            ds *= 2
    resnet("mid_block_resnets_0", "middle_block.0", False)
    attention("mid_block_attentions_0", "middle_block.1")
    resnet("mid_block_resnets_1", "middle_block.2", False)
    for i in range(nlev):                                        # up blocks, i = 0 the deepest
        level = nlev - 1 - i
        has_attn = ds in cfg.attention_resolutions
        for j in range(n + 1):
            b = (n + 1) * i + j
            resnet(f"up_blocks_{i}_resnets_{j}", f"output_blocks.{b}.0", True)        # (a concatenation never keeps its width)
            ch = mult[level]
            skips.pop()
            if has_attn:
                attention(f"up_blocks_{i}_attentions_{j}", f"output_blocks.{b}.1")
        if level:
            out.append((f"up_blocks_{i}_upsamplers_0_conv", f"output_blocks.{(n + 1) * i + n}.{2 if has_attn else 1}.conv"))
            ds //= 2
    return out


def kohya_text_names(layers):
    out = []
    for i in range(layers):
        for k, p in (("self_attn_q_proj", "self_attn.q_proj"), ("self_attn_k_proj", "self_attn.k_proj"), ("self_attn_v_proj", "self_attn.v_proj"),
                     ("self_attn_out_proj", "self_attn.out_proj"), ("mlp_fc1", "mlp.fc1"), ("mlp_fc2", "mlp.fc2")):
            out.append((f"text_model_encoder_layers_{i}_{k}", f"transformer.text_model.encoder.layers.{i}.{p}"))
    return out
