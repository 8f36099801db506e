"""Stand-ins for the attention-processor classes of the reference and of diffusers, which cannot be imported here.  Written fresh: class
names, constructor keywords and the attributes the engine reads -- no behaviour.  The engine recognises processors by class name and
attributes (mvedit_amd/attn_processors.py), so these are what it sees when the reference installs the real ones."""
import torch


class AttnProcessor2_0(torch.nn.Module):
    """diffusers / ip_adapter plain processor: no state."""


class IPAttnProcessor(torch.nn.Module):
    def __init__(self, hidden_size, cross_attention_dim=None, scale=1.0, num_tokens=4):
        super().__init__()
        self.hidden_size, self.cross_attention_dim, self.scale, self.num_tokens = hidden_size, cross_attention_dim, scale, num_tokens
        self.to_k_ip = torch.nn.Linear(cross_attention_dim or hidden_size, hidden_size, bias=False)
        self.to_v_ip = torch.nn.Linear(cross_attention_dim or hidden_size, hidden_size, bias=False)


class CNAttnProcessor:
    def __init__(self, num_tokens=4):
        self.num_tokens = num_tokens


class CrossImageAttnProcWrapper(torch.nn.Module):
    def __init__(self, base_attn_proc):
        super().__init__()
        self.base_attn_proc = base_attn_proc


class ReferenceOnlyAttnProc(torch.nn.Module):
    def __init__(self, chained_proc, enabled=False, name=None):
        super().__init__()
        self.enabled, self.chained_proc, self.name = enabled, chained_proc, name


class LoRAAttnProcessor(torch.nn.Module):
    """A processor the engine does not implement."""


def hidden_size(cfg, name):
    """Width of the attention layer `name` (the rule of ip_adapter.py:90-97, restated)."""
    ch = cfg['block_out_channels']
    if name.startswith('mid_block'):
        return ch[-1]
    i = int(name.split('.')[1])
    return list(reversed(ch))[i] if name.startswith('up_blocks') else ch[i]


def ip_table(cfg, names, num_tokens=16, scale=1.0, wrap=None):
    """IPAttnProcessor on every attn2, a plain processor on every attn1 (what IPAdapter.set_ip_adapter installs); wrap(proc) around each."""
    wrap = wrap or (lambda p: p)
    return {n: wrap(AttnProcessor2_0() if n.endswith('attn1.processor') else
                    IPAttnProcessor(hidden_size(cfg, n), cfg['cross_attention_dim'], scale=scale, num_tokens=num_tokens)) for n in names}


def ip_checkpoint(ip_sd, names):
    """The `ip_adapter` part of an IP-Adapter checkpoint: integer keys in TABLE order (`<index>.to_k_ip.weight`), built from a state dict with
    the diffusers names `<block>.attn2.processor.to_{k,v}_ip.weight` (oracle.unet_oracle.make_ip_state_dict)."""
    ck = {}
    for i, n in enumerate(names):
        if n.endswith('attn2.processor'):
            for kv in ('to_k_ip', 'to_v_ip'):
                ck[f'{i}.{kv}.weight'] = ip_sd[f'{n}.{kv}.weight']
    return ck
