"""`nvdiffrast.torch` for the reference on gfx950: nvdiffrast's public names and argument order on the native mesh kernels.

The reference's own MeshRenderer (lib/models/decoders/mesh_renderer/base_mesh_renderer.py) does `import nvdiffrast.torch as dr` at module
level, builds `dr.RasterizeCudaContext()` in its constructor (:204) and renders through `dr.rasterize / interpolate / texture / antialias`
(:241-298, :407-588).  `mvedit_amd.dropin.install()` seeds this module under that name.

Forward results are those of `mvedit_amd.mesh_ops` (same kernels).  Gradients, first order:

    rasterize    pos   <- rast (u, v, z/w) and rast_db               mve_rasterize_backward, mve_rasterize_db_backward
    interpolate  attr, rast (u, v), rast_db <- out and out_da        mve_interpolate_backward(_rast), mve_interpolate_da_backward
    texture      tex, uv, uv_da <- out                               mve_texture_*_backward, mve_texture_grad_uv
    antialias    color, pos <- out                                   mve_antialias_backward(_pos)

i.e. unlike `mesh_ops.texture` (which refuses a uv that requires grad) the path from a texture fetch back to the geometry exists here.  The
gradient is the derivative of this package's own forward formulas (csrc/texmip_core.h, oracle/texture_mip_oracle.py) with every pixel's
triangle, the bilinear tap indices and the mip level pair held fixed; nvdiffrast itself cannot be run on this hardware, so no parity with its
backward is claimed.  Under create_graph=True the gradients carry a node that raises when differentiated again.

Not built -- NotImplementedError naming the argument, never a fallback: range mode (`ranges=`, 2-D `pos` / `attr`), `boundary_mode` other
than 'wrap', `filter_mode` 'nearest' / 'linear-mipmap-nearest', cube maps, `mip_level_bias`, a prebuilt `mip=`, CPU tensors.
"""
import torch

from .. import _lib, mesh_ops

__all__ = ['RasterizeCudaContext', 'RasterizeGLContext', 'rasterize', 'interpolate', 'texture', 'antialias',
           'antialias_construct_topology_hash', 'get_log_level', 'set_log_level']

_log_level = 1


def get_log_level():
    """nvdiffrast's logging knob: the value is kept, nothing reads it."""
    return _log_level


def set_log_level(level):
    global _log_level
    _log_level = int(level)


class RasterizeCudaContext:
    """dr.RasterizeCudaContext(device=None): a plain, copyable object (the rasteriser keeps no state between calls)."""

    def __init__(self, device=None):
        self.device = device
        self.output_db = True


class RasterizeGLContext:
    """dr.RasterizeGLContext(output_db=True, mode='automatic', device=None): there is no OpenGL path -- it rasterises with the same HIP
    kernels; `output_db=False` makes `rasterize` return an empty rast_db as nvdiffrast does."""

    def __init__(self, output_db=True, mode='automatic', device=None):
        assert mode in ('automatic', 'manual'), mode
        self.output_db, self.mode, self.device = bool(output_db), mode, device

    def set_context(self):
        pass

    def release_context(self):
        pass


class _SecondOrderError(torch.autograd.Function):
    """Identity on a first-order gradient computed with create_graph=True; differentiating it raises (instead of a silent zero).  `deps` are
    the tensors the gradient depends on (the op's inputs and the incoming gradients): they tie the node into the graph, so that it is reached
    whichever input the second differentiation asks for."""

    @staticmethod
    def forward(ctx, t, *deps):
        return t.clone()

    @staticmethod
    def backward(ctx, g):
        raise RuntimeError('mvedit_amd.nvdiffrast.torch: second-order gradients are not implemented: the backward is once-differentiable')


def _first_order(backward):
    """The backward of every Function here: runs without a graph; under create_graph=True its results carry a node that raises."""
    def wrapped(ctx, *grads):
        create_graph = torch.is_grad_enabled()
        with torch.no_grad():
            out = backward(ctx, *[None if g is None else g.detach().float().contiguous() for g in grads])
        if create_graph:
            deps = [t for t in tuple(ctx.saved_tensors) + tuple(grads) if torch.is_tensor(t) and t.requires_grad]
            out = tuple(_SecondOrderError.apply(o.requires_grad_(), *deps) if torch.is_tensor(o) else o for o in out)
        return out
    return staticmethod(wrapped)


def _need_cuda(fn, **tensors):
    for name, t in tensors.items():
        if t is not None and not t.is_cuda:
            raise NotImplementedError(f'{fn}: {name} is a CPU tensor; only GPU tensors are implemented (there is no CPU path)')


def _f32(t):
    return t.float().contiguous()


def _i32(t):
    return t.to(torch.int32).contiguous()


# ---------------------------------------------------------------------------------------------------------------------------------------
class _RasterizeFn(torch.autograd.Function):
    """(rast, rast_db) with the gradient of both w.r.t. pos: rast_db depends on the triangle's clip (x, y, w) directly and on the stored
    (u, v), whose own dependence on pos is mve_rasterize_backward's."""

    @staticmethod
    def forward(ctx, pos, tri, h, w, grad_db):
        rast = mesh_ops._rasterize_raw(pos, tri, (h, w))
        db = mesh_ops.rasterize_db(pos, tri, rast)
        ctx.save_for_backward(pos, tri, rast)
        ctx.set_materialize_grads(False)
        if not grad_db:
            ctx.mark_non_differentiable(db)
        return rast, db

    @_first_order
    def backward(ctx, g_rast, g_db):
        pos, tri, rast = ctx.saved_tensors
        if g_rast is None and g_db is None:
            return None, None, None, None, None
        B, V, _ = pos.shape
        _, h, w, _ = rast.shape
        g_pos = torch.zeros_like(pos)
        with torch.cuda.device(pos.device):
            if g_db is not None:
                via_uv = torch.empty_like(rast)
                _lib.call('mve_rasterize_db_backward', _lib.ptr(pos), B, V, _lib.ptr(tri), tri.shape[0], _lib.ptr(rast), h, w, _lib.ptr(g_db),
                          _lib.ptr(g_pos), _lib.ptr(via_uv), _lib.stream_ptr(pos.device))
                g_rast = via_uv if g_rast is None else g_rast + via_uv
            _lib.call('mve_rasterize_backward', _lib.ptr(pos), B, V, _lib.ptr(tri), tri.shape[0], h, w, _lib.ptr(rast), _lib.ptr(g_rast),
                      _lib.ptr(g_pos), _lib.stream_ptr(pos.device))
        return g_pos, None, None, None, None


def rasterize(glctx, pos, tri, resolution, ranges=None, grad_db=True):
    """dr.rasterize, instanced mode: pos [B,V,4] clip space, tri [F,3] -> (rast [B,h,w,4] = (u, v, z/w, triangle_id + 1), rast_db [B,h,w,4] =
    (du/dX, du/dY, dv/dX, dv/dY); [B,h,w,0] for a GL context built with output_db=False).  With grad_db=False rast_db is detached."""
    if ranges is not None:
        raise NotImplementedError('rasterize: ranges= (range mode) is not implemented; only instanced mode (pos [B,V,4]) is')
    if pos.dim() != 3:
        raise NotImplementedError(f'rasterize: pos of shape {tuple(pos.shape)} (range mode) is not implemented; only instanced mode (pos [B,V,4]) is')
    assert pos.shape[-1] == 4 and tri.dim() == 2 and tri.shape[1] == 3 and len(resolution) == 2
    _need_cuda('rasterize', pos=pos, tri=tri)
    rast, db = _RasterizeFn.apply(_f32(pos), _i32(tri), int(resolution[0]), int(resolution[1]), bool(grad_db))
    if not getattr(glctx, 'output_db', True):
        db = rast.new_zeros(rast.shape[:-1] + (0,))
    return rast, db


# ---------------------------------------------------------------------------------------------------------------------------------------
class _InterpolateFn(torch.autograd.Function):
    """(out, out_da for every attribute); rast_db None: out_da is empty and carries no gradient."""

    @staticmethod
    def forward(ctx, attr, rast, tri, rast_db):
        out = mesh_ops._interpolate_raw(attr, rast, tri)
        if rast_db is None:
            da = out.new_zeros(out.shape[:-1] + (0,))
            ctx.mark_non_differentiable(da)
        else:
            da = mesh_ops.interpolate_da(attr, rast, rast_db, tri)
        ctx.save_for_backward(attr, rast, tri, rast_db)
        ctx.set_materialize_grads(False)
        return out, da

    @_first_order
    def backward(ctx, g_out, g_da):
        attr, rast, tri, rast_db = ctx.saved_tensors
        Ba, V, A = attr.shape
        B, h, w, _ = rast.shape
        dev, F = rast.device, tri.shape[0]
        need_attr, need_rast, need_db = ctx.needs_input_grad[0], ctx.needs_input_grad[1], rast_db is not None and ctx.needs_input_grad[3]
        g_attr = torch.zeros_like(attr) if need_attr else None
        g_rast = g_db = None
        with torch.cuda.device(dev):
            if g_out is not None and need_attr:
                _lib.call('mve_interpolate_backward', _lib.ptr(g_out), Ba, V, A, _lib.ptr(rast), B, h, w, _lib.ptr(tri), F, _lib.ptr(g_attr),
                          _lib.stream_ptr(dev))
            if g_out is not None and need_rast:
                g_rast = torch.empty_like(rast)
                _lib.call('mve_interpolate_backward_rast', _lib.ptr(attr), Ba, V, A, _lib.ptr(rast), B, h, w, _lib.ptr(tri), F, _lib.ptr(g_out),
                          _lib.ptr(g_rast), _lib.stream_ptr(dev))
            if g_da is not None and rast_db is not None and (need_attr or need_db):
                g_db = torch.empty_like(rast_db) if need_db else None
                _lib.call('mve_interpolate_da_backward', _lib.ptr(attr), Ba, V, A, _lib.ptr(rast), _lib.ptr(rast_db), B, h * w, _lib.ptr(tri), F,
                          _lib.ptr(g_da), _lib.ptr(g_db), _lib.ptr(g_attr), _lib.stream_ptr(dev))
        return g_attr, g_rast, None, g_db


def interpolate(attr, rast, tri, rast_db=None, diff_attrs=None):
    """dr.interpolate, instanced mode: attr [1 or B, V, A] -> (out [B,h,w,A], out_da [B,h,w,2K]) with out_da = (dA/dX, dA/dY) of the K
    attributes `diff_attrs` names ('all' or a list of indices); [B,h,w,0] without rast_db / diff_attrs."""
    if attr.dim() != 3:
        raise NotImplementedError(f'interpolate: attr of shape {tuple(attr.shape)} (range mode) is not implemented; only instanced mode '
                                  '(attr [1 or B, V, A]) is')
    if diff_attrs is not None and not (isinstance(diff_attrs, str) and diff_attrs == 'all'):
        diff_attrs = [int(i) for i in diff_attrs]
        assert all(0 <= i < attr.shape[-1] for i in diff_attrs), diff_attrs
    if diff_attrs is not None and len(diff_attrs) > 0 and rast_db is None:
        raise ValueError('interpolate: diff_attrs needs rast_db')
    assert rast.dim() == 4 and rast.shape[-1] == 4 and tri.dim() == 2 and tri.shape[1] == 3
    _need_cuda('interpolate', attr=attr, rast=rast, tri=tri, rast_db=rast_db)
    want_da = rast_db is not None and diff_attrs is not None and len(diff_attrs) > 0
    if want_da and tuple(rast_db.shape) != tuple(rast.shape):
        raise ValueError(f'interpolate: rast_db of shape {tuple(rast_db.shape)} does not match rast {tuple(rast.shape)}')
    out, da = _InterpolateFn.apply(_f32(attr), _f32(rast), _i32(tri), _f32(rast_db) if want_da else None)
    if want_da and diff_attrs != 'all':
        B, h, w, _ = out.shape
        da = da.reshape(B, h, w, attr.shape[-1], 2)[..., diff_attrs, :].reshape(B, h, w, 2 * len(diff_attrs))
    return out, da


# ---------------------------------------------------------------------------------------------------------------------------------------
class _TextureFn(torch.autograd.Function):
    """uv_da None: bilinear; otherwise trilinear over the box-filtered level stack.  No rast: every pixel fetches at its uv."""

    @staticmethod
    def forward(ctx, tex, uv, uv_da, max_mip_level):
        ctx.save_for_backward(tex, uv, uv_da)
        ctx.max_mip_level = max_mip_level
        if uv_da is None:
            return mesh_ops._texture_raw(tex, uv, None)
        mips, lv = mesh_ops.build_mips(tex, max_mip_level)
        return mesh_ops._texture_mip_raw(tex, mips, lv, uv, uv_da, None)

    @_first_order
    def backward(ctx, g):
        tex, uv, uv_da = ctx.saved_tensors
        Bt, H, W, C = tex.shape
        n, h, w, _ = uv.shape
        dev = uv.device
        mip = uv_da is not None
        lv = mesh_ops._mip_levels(H, W, ctx.max_mip_level) if mip else 0
        g_tex = g_uv = g_da = None
        with torch.cuda.device(dev):
            if ctx.needs_input_grad[0]:
                if mip:
                    g_tex = torch.empty_like(tex)
                    g_mips = torch.empty(Bt, max(1, _lib.raw('mve_mip_texels')(H, W, lv) * C), dtype=torch.float32, device=dev)
                    _lib.call('mve_texture_mip_backward', _lib.ptr(g), Bt, H, W, C, lv, _lib.ptr(uv), _lib.ptr(uv_da), None, n, h, w,
                              _lib.ptr(g_tex), _lib.ptr(g_mips), _lib.stream_ptr(dev))
                else:
                    g_tex = torch.zeros_like(tex)
                    _lib.call('mve_texture_bilinear_backward', _lib.ptr(g), Bt, H, W, C, _lib.ptr(uv), None, n, h, w, _lib.ptr(g_tex),
                              _lib.stream_ptr(dev))
            need_uv, need_da = ctx.needs_input_grad[1], mip and ctx.needs_input_grad[2]
            if need_uv or need_da:
                mips = mesh_ops.build_mips(tex, ctx.max_mip_level)[0] if mip else None        # rebuilt rather than kept alive since the forward
                g_uv = torch.empty_like(uv) if need_uv else None
                g_da = torch.empty_like(uv_da) if need_da else None
                _lib.call('mve_texture_grad_uv', _lib.ptr(tex), _lib.ptr(mips), Bt, H, W, C, lv, _lib.ptr(uv), _lib.ptr(uv_da), _lib.ptr(g),
                          n, h, w, _lib.ptr(g_uv), _lib.ptr(g_da), _lib.stream_ptr(dev))
        return g_tex, g_uv, g_da, None


def texture(tex, uv, uv_da=None, mip_level_bias=None, mip=None, filter_mode='auto', boundary_mode='wrap', max_mip_level=None):
    """dr.texture: tex [1 or n, H, W, C], uv [n,h,w,2], uv_da [n,h,w,4] -> [n,h,w,C]; 'auto' is 'linear-mipmap-linear' with uv_da, else
    'linear'.  Wrap addressing.  There is no rast argument: empty pixels fetch at their uv (0, 0), as with nvdiffrast."""
    if mip_level_bias is not None:
        raise NotImplementedError('texture: mip_level_bias is not implemented')
    if mip is not None:
        raise NotImplementedError('texture: a prebuilt mip= stack is not implemented (the level stack is built per call)')
    if boundary_mode != 'wrap':
        raise NotImplementedError(f"texture: boundary_mode={boundary_mode!r} is not implemented; only 'wrap' is (no clamp / zero / cube maps)")
    if filter_mode == 'auto':
        filter_mode = 'linear-mipmap-linear' if uv_da is not None else 'linear'
    if filter_mode not in ('linear', 'linear-mipmap-linear'):
        raise NotImplementedError(f"texture: filter_mode={filter_mode!r} is not implemented; only 'linear' and 'linear-mipmap-linear' are")
    if tex.dim() != 4 or uv.dim() != 4 or uv.shape[-1] != 2:
        raise NotImplementedError(f'texture: tex {tuple(tex.shape)} / uv {tuple(uv.shape)}: only 2-D textures [1 or n, H, W, C] with uv [n,h,w,2] are '
                                  'implemented (no cube maps)')
    if filter_mode == 'linear-mipmap-linear':
        if uv_da is None:
            raise ValueError("texture: filter_mode='linear-mipmap-linear' needs uv_da")
        assert tuple(uv_da.shape) == tuple(uv.shape[:-1]) + (4,), (uv_da.shape, uv.shape)
    else:
        uv_da = None
    assert tex.shape[0] in (1, uv.shape[0]), (tex.shape, uv.shape)
    _need_cuda('texture', tex=tex, uv=uv, uv_da=uv_da)
    return _TextureFn.apply(_f32(tex), _f32(uv), _f32(uv_da) if uv_da is not None else None,
                            None if max_mip_level is None else int(max_mip_level))


# ---------------------------------------------------------------------------------------------------------------------------------------
def antialias_construct_topology_hash(tri):
    """What `antialias(topology_hash=)` accepts: opp [F,3] int32, the vertex opposite to every edge in the adjacent triangle."""
    _need_cuda('antialias_construct_topology_hash', tri=tri)
    return mesh_ops.edge_opposites(tri)


class _AntialiasFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, color, rast, pos, tri, opp, boost):
        ctx.save_for_backward(color if ctx.needs_input_grad[2] else None, rast, pos, tri, opp)
        ctx.boost = boost
        return mesh_ops._antialias_raw(color, rast, pos, tri, opp)

    @_first_order
    def backward(ctx, g):
        color, rast, pos, tri, opp = ctx.saved_tensors
        B, h, w, C = g.shape
        dev, V, F = g.device, pos.shape[1], tri.shape[0]
        g_in = g_pos = None
        with torch.cuda.device(dev):
            if ctx.needs_input_grad[0]:
                g_in = torch.empty_like(g)
                _lib.call('mve_antialias_backward', _lib.ptr(g), B, h, w, C, _lib.ptr(rast), _lib.ptr(pos), V, _lib.ptr(tri), F, _lib.ptr(opp),
                          _lib.ptr(g_in), _lib.stream_ptr(dev))
            if ctx.needs_input_grad[2]:
                g_pos = torch.zeros_like(pos)
                _lib.call('mve_antialias_backward_pos', _lib.ptr(color), _lib.ptr(g), B, h, w, C, _lib.ptr(rast), _lib.ptr(pos), V, _lib.ptr(tri), F,
                          _lib.ptr(opp), _lib.ptr(g_pos), _lib.stream_ptr(dev))
                if ctx.boost != 1.0:
                    g_pos = g_pos * ctx.boost
        return g_in, None, g_pos, None, None, None


def antialias(color, rast, pos, tri, topology_hash=None, pos_gradient_boost=1.0):
    """dr.antialias, instanced mode: color [B,h,w,C] -> same shape.  Gradients to color and (the silhouette term) to pos, the latter scaled by
    pos_gradient_boost."""
    if pos.dim() != 3:
        raise NotImplementedError(f'antialias: pos of shape {tuple(pos.shape)} (range mode) is not implemented; only instanced mode (pos [B,V,4]) is')
    assert color.dim() == 4 and rast.dim() == 4 and tuple(color.shape[:3]) == tuple(rast.shape[:3]) and tri.dim() == 2 and tri.shape[1] == 3
    _need_cuda('antialias', color=color, rast=rast, pos=pos, tri=tri, topology_hash=topology_hash)
    tri = _i32(tri)
    opp = mesh_ops.edge_opposites(tri) if topology_hash is None else _i32(topology_hash)
    assert tuple(opp.shape) == tuple(tri.shape), (opp.shape, tri.shape)
    return _AntialiasFn.apply(_f32(color), _f32(rast.detach()), _f32(pos), tri, opp, float(pos_gradient_boost))
