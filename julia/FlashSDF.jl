# FlashSDF.jl — the Julia drop-in for Flash.jl's residual path over libflashsdf
# (include/flashsdf.h). To be `include`d from src/Flash.jl after
# gradientdescent.jl; src/tracking.jl:16 then builds
#     cost = FlashSDF.GPUCost(manipulator, sensed_points)
# instead of CostFunctor(manipulator, sensed_points) — the same callable with
# Float64 or ForwardDiff.Dual input (src/gradientdescent.jl:49-57).
#
# Julia 0.5 syntax, like the reference (REQUIRE.dev:1). Julia is not installed
# in this image, so this file is not executed here; its ccall signatures and C
# struct layouts are checked against include/flashsdf.h by
# tests/test_julia_shim.py, and its arithmetic mirrors the tested Python host
# (flash/gradientdescent.py, flash/rbf.py).
#
# How the gradient is formed. The reference differentiates the whole cost with
# ForwardDiff chunk passes: ⌈n/9⌉ Dual evaluations of every (point, surface)
# pair (examples/irb_and_squishable.ipynb:482-485). Here the per-point work runs
# ONCE per distinct value(x) on the GPU, which returns the cost and its
# first-order sensitivities to the scene geometry:
#   * per convex surface k: F_k = Σ 2d∇d, M_k = Σ 2d p×∇d (accum[1+6k..]), so
#     that a world twist (ω, v) of the surface changes the cost by
#     δc = −(ω·M_k + v·F_k);
#   * per RBF skin: λ = Σ 2s ∂s/∂(w, a, b) and E_i = Σ 2s ∂s/∂c_i.
# Everything upstream of the GPU — forward kinematics (RigidBodyDynamics,
# src/Flash.jl:248), normalize! (src/gradientdescent.jl:30), the deformed
# surface points (src/Flash.jl:143-201) and the RBF weight solve
# (src/Flash.jl:212) — is evaluated by the reference's own code in the Dual
# number type, and the chunk's partials are contracted with those
# sensitivities. The result is the first-order Dual the reference would
# produce, from one residual pass instead of ⌈n/9⌉.

module FlashSDF

import Flash
import Flash: Manipulator, ManipulatorState, ConvexGeometry, InterpolatingGeometry
import Flash.GradientDescent: unflatten!, default_deformation_cost_weight
import Base: normalize!   # extended for MechanismState in src/gradientdescent.jl:19-26
using RigidBodyDynamics
using CoordinateTransformations
import StaticArrays: SVector
import GeometryTypes
import ForwardDiff
import ForwardDiff: Dual, value, partials

const lib = get(ENV, "FLASHSDF_LIB", "libflashsdf")

const FSDF_SURFACE_HULL = Int32(0)
const FSDF_SURFACE_RBF = Int32(1)

# C structs of include/flashsdf.h (field order and types as declared there)
immutable Opts          # fsdf_opts
    device::Int32
    precision::Int32
    sort_points::Int32
    cull::Int32
end

immutable Hull          # fsdf_hull
    n_vertices::Int32
    n_faces::Int32
    vertices::Ptr{Float64}
    faces::Ptr{Int32}
    planes::Ptr{Float64}
end

immutable Surface       # fsdf_surface
    kind::Int32
    n_centers::Int32
    hull::Hull
end

last_error(ptr::Ptr{Void}) = unsafe_string(ccall((:fsdf_last_error, lib), Cstring, (Ptr{Void},), ptr))
check(ptr::Ptr{Void}, st::Cint, what) = st == 0 || error("flashsdf $what (status $st): ", last_error(ptr))

"conv(points) for a 3×n vertex matrix → (3×m vertices, 3×f zero-based faces, 4×f
planes): the shape EnhancedGJK's NeighborMesh support function sees (src/models.jl:152)."
function convex_hull(points::Matrix{Float64})
    n = size(points, 2)
    cap = max(2n - 4, 4)
    v = zeros(3, max(n, 4)); f = zeros(Int32, 3, cap); p = zeros(4, cap)
    nv = Ref{Int32}(0); nf = Ref{Int32}(0)
    st = ccall((:fsdf_convex_hull, lib), Cint,
               (Ptr{Float64}, Int32, Ref{Int32}, Ptr{Float64}, Ref{Int32}, Ptr{Int32}, Ptr{Float64}),
               points, n, nv, v, nf, f, p)
    st == 0 || error("fsdf_convex_hull: status $st")
    v[:, 1:nv[]], f[:, 1:nf[]], p[:, 1:nf[]]
end

"One device context holding the manipulator's surfaces (uploaded once)."
type Context
    ptr::Ptr{Void}
    manipulator::Manipulator
    S::Int
    accum_len::Int
    prefetched::Any   # the cloud fsdf_prefetch_points is copying (rooted until consumed)
end
Context(ptr, manip, S, accum_len) = Context(ptr, manip, S, accum_len, nothing)

function Context(manip::Manipulator; device::Integer=0, precision::Integer=64, sort_points::Bool=true)
    ref = Ref{Ptr{Void}}(C_NULL)
    st = ccall((:fsdf_create, lib), Cint, (Ref{Ptr{Void}}, Ref{Opts}),
               ref, Opts(device, precision, sort_points ? 1 : 0, 1))
    st == 0 || error("fsdf_create: no usable HIP device (status $st; libflashsdf has no CPU fallback)")
    keep = Any[]          # the hull arrays must outlive fsdf_set_surfaces (it copies them)
    descs = Surface[]
    for s in manip.surfaces
        if isa(s, ConvexGeometry)
            # the vertex set Flash.surface_points(::ConvexGeometry) uses (src/Flash.jl:143-148)
            verts = GeometryTypes.vertices(s.geometry)
            V = Float64[v[i] for i in 1:3, v in verts]
            hv, hf, hp = convex_hull(V)
            push!(keep, hv, hf, hp)
            push!(descs, Surface(FSDF_SURFACE_HULL, 0,
                                 Hull(size(hv, 2), size(hf, 2), pointer(hv), pointer(hf), pointer(hp))))
        else
            n = length(s.surface_points) + length(s.skeleton_points)
            push!(descs, Surface(FSDF_SURFACE_RBF, n, Hull(0, 0, C_NULL, C_NULL, C_NULL)))
        end
    end
    check(ref[], ccall((:fsdf_set_surfaces, lib), Cint, (Ptr{Void}, Ptr{Surface}, Int32),
                       ref[], descs, length(descs)), "set_surfaces")
    len = Ref{Int32}(0)
    check(ref[], ccall((:fsdf_accum_len, lib), Cint, (Ptr{Void}, Ref{Int32}), ref[], len), "accum_len")
    ctx = Context(ref[], manip, length(descs), len[])
    finalizer(ctx, c -> ccall((:fsdf_destroy, lib), Cint, (Ptr{Void},), c.ptr))
    ctx
end

"Upload the sensed cloud once per frame (CostFunctor keeps it by reference,
src/gradientdescent.jl:41-47). Vector{SVector{3,Float64}} is a contiguous AoS
buffer of 3n doubles: passed zero-copy."
function set_points!{T}(ctx::Context, pts::AbstractVector{SVector{3, T}})
    P = convert(Vector{SVector{3, Float64}}, pts)
    check(ctx.ptr, ccall((:fsdf_set_points, lib), Cint, (Ptr{Void}, Ptr{Float64}, Int64),
                         ctx.ptr, reinterpret(Float64, P), length(P)), "set_points")
end

"Start the NEXT frame's upload now (fsdf_prefetch_points: a copy on the context's
own stream, under the current frame's iterations — overlapped when the buffer is
page-locked); set_points_prefetched! makes it resident. The buffer is rooted in the
context until then and must not change."
function prefetch_points!{T}(ctx::Context, pts::AbstractVector{SVector{3, T}})
    P = convert(Vector{SVector{3, Float64}}, pts)
    check(ctx.ptr, ccall((:fsdf_prefetch_points, lib), Cint, (Ptr{Void}, Ptr{Float64}, Int64),
                         ctx.ptr, reinterpret(Float64, P), length(P)), "prefetch_points")
    ctx.prefetched = P
end

function set_points_prefetched!(ctx::Context)
    check(ctx.ptr, ccall((:fsdf_set_points_prefetched, lib), Cint, (Ptr{Void},), ctx.ptr), "set_points_prefetched")
    ctx.prefetched = nothing
end

"""
The depth sensor's rays (src/depthsensors.jl DepthSensor: `rays[rows, cols]`, camera frame), kept
on the device as one direction per pixel (fsdf_set_sensor). `z_depth = false`: a frame's depths
are distances along the rays, the reference's model; `true`: camera-frame z. The C side reads the
rays row-major, so the column-major matrix is transposed here.
"""
function set_sensor!{T}(ctx::Context, rays::AbstractMatrix{SVector{3, T}}; z_depth::Bool=false)
    rows, cols = size(rays)
    R = convert(Vector{SVector{3, Float64}}, vec(permutedims(rays, (2, 1))))
    check(ctx.ptr, ccall((:fsdf_set_sensor, lib), Cint, (Ptr{Void}, Ptr{Float64}, Int32, Int32, Int32),
                         ctx.ptr, reinterpret(Float64, R), Int32(rows), Int32(cols), Int32(z_depth ? 1 : 0)), "set_sensor")
end

"""
One depth frame in place of raycast_points + set_points! (src/depthsensors.jl:99-113): `depths[rows, cols]`
over the sensor's rays and the sensor's pose (R [3, 3], t [3]) in the world; the device back-projects
the pixels with near <= scale * depth <= far (finite, > 0) and compacts them in row-major order
(fsdf_set_depth_f64). `depth_pixels` names each resident point's pixel.
"""
function set_depth!(ctx::Context, depths::AbstractMatrix{Float64}, R::AbstractMatrix, t::AbstractVector;
                    near::Float64=0.0, far::Float64=Inf, scale::Float64=1.0)
    D = convert(Vector{Float64}, vec(permutedims(depths, (2, 1))))
    pose = convert(Vector{Float64}, vcat(vec(permutedims(R, (2, 1))), t))
    range = Float64[near, far, scale]
    check(ctx.ptr, ccall((:fsdf_set_depth_f64, lib), Cint, (Ptr{Void}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}),
                         ctx.ptr, D, pose, range), "set_depth")
end

"The 1-based (row, col) of every point of the resident depth frame, in the points' order (fsdf_get_depth_pixels)."
function depth_pixels(ctx::Context, cols::Integer)
    n = Ref{Int64}(0)
    check(ctx.ptr, ccall((:fsdf_get_depth_pixels, lib), Cint, (Ptr{Void}, Ptr{Int32}, Ref{Int64}),
                         ctx.ptr, C_NULL, n), "get_depth_pixels")
    pix = zeros(Int32, n[])
    check(ctx.ptr, ccall((:fsdf_get_depth_pixels, lib), Cint, (Ptr{Void}, Ptr{Int32}, Ref{Int64}),
                         ctx.ptr, pix, n), "get_depth_pixels")
    [(div(p, cols) + 1, rem(p, cols) + 1) for p in pix]
end

"""
The free-space samples every later set_depth! sends after its observed points (fsdf_set_free_space):
`samples` = J in 1..16 per sending pixel on every `stride`-th row and column, at ranges
s - gap - (j - 1) * spacing along the pixel's ray (a miss, when miss_range > 0: from miss_range), only
where the last one stays in front of the camera. The frame then sets the split of the resident
cloud itself: the samples count only where the model covers them (d* < 0). `samples = 0` turns it off.
"""
function set_free_space!(ctx::Context, samples::Integer, stride::Integer=1; gap::Float64=0.02,
                         spacing::Float64=0.05, miss_range::Float64=0.0)
    lengths = Float64[gap, spacing, miss_range]
    check(ctx.ptr, ccall((:fsdf_set_free_space, lib), Cint, (Ptr{Void}, Int32, Int32, Ptr{Float64}),
                         ctx.ptr, Int32(samples), Int32(stride), lengths), "set_free_space")
end

"(samples, stride, gap, spacing, miss_range) as the library holds them; samples 0: off (fsdf_get_free_space)."
function free_space(ctx::Context)
    samples, stride, lengths = Ref{Int32}(0), Ref{Int32}(0), zeros(Float64, 3)
    check(ctx.ptr, ccall((:fsdf_get_free_space, lib), Cint, (Ptr{Void}, Ref{Int32}, Ref{Int32}, Ptr{Float64}),
                         ctx.ptr, samples, stride, lengths), "get_free_space")
    (Int(samples[]), Int(stride[]), lengths[1], lengths[2], lengths[3])
end

"""
Points n_surface + 1 : n of the resident cloud, in the order given to set_points!, are free-space
samples: positions known to be empty, which count only where the model covers them (fsdf_set_free_split;
the robust path, also without a loss). `n_surface` = n or a negative value clears it; every new cloud does.
"""
set_free_split!(ctx::Context, n_surface::Integer) =
    check(ctx.ptr, ccall((:fsdf_set_free_split, lib), Cint, (Ptr{Void}, Int64), ctx.ptr, Int64(n_surface)),
          "set_free_split")

"n_surface of the resident cloud, or `nothing` when no split is set (fsdf_get_free_split)."
function free_split(ctx::Context)
    n, set = Ref{Int64}(0), Ref{Int32}(0)
    check(ctx.ptr, ccall((:fsdf_get_free_split, lib), Cint, (Ptr{Void}, Ref{Int64}, Ref{Int32}), ctx.ptr, n, set),
          "get_free_split")
    set[] == 0 ? nothing : Int(n[])
end

"""
The voxel grid that set_points_voxel! and every later set_depth! thin their cloud through
(fsdf_set_voxel_grid, with the size by reference): one centroid per occupied cell of side `size`
counted from `origin`, in ascending cell order; `count_weights = true`: the cells' populations become
the point weights. `size = 0` turns it off. Kept over frames and model swaps.
"""
set_voxel_grid!(ctx::Context, size::Real; origin::AbstractVector=[0.0, 0.0, 0.0], count_weights::Bool=true) =
    check(ctx.ptr, ccall((:fsdf_set_voxel_grid_ref, lib), Cint, (Ptr{Void}, Ptr{Float64}, Ptr{Float64}, Int32),
                         ctx.ptr, Float64[size], convert(Vector{Float64}, origin), Int32(count_weights ? 1 : 0)),
          "set_voxel_grid")

"set_points! through the context's voxel grid: the cells' centroids become the resident cloud (fsdf_set_points_voxel)."
function set_points_voxel!{T}(ctx::Context, points::AbstractVector{SVector{3, T}})
    P = convert(Vector{SVector{3, Float64}}, points)
    check(ctx.ptr, ccall((:fsdf_set_points_voxel, lib), Cint, (Ptr{Void}, Ptr{Float64}, Int64),
                         ctx.ptr, reinterpret(Float64, P), length(P)), "set_points_voxel")
end

"""
Of the resident voxel cloud: (centroids, counts, cells [3, m], number of input points, number dropped as
non-finite), the voxels in the cloud's order (fsdf_get_voxels).
"""
function voxels(ctx::Context)
    m, n_in, dropped = Ref{Int64}(0), Ref{Int64}(0), Ref{Int64}(0)
    check(ctx.ptr, ccall((:fsdf_get_voxels, lib), Cint,
                         (Ptr{Void}, Ptr{Float64}, Ptr{Int32}, Ptr{Int32}, Ref{Int64}, Ref{Int64}, Ref{Int64}),
                         ctx.ptr, C_NULL, C_NULL, C_NULL, m, n_in, dropped), "get_voxels")
    xyz, count, cell = zeros(Float64, 3, m[]), zeros(Int32, m[]), zeros(Int32, 3, m[])
    check(ctx.ptr, ccall((:fsdf_get_voxels, lib), Cint,
                         (Ptr{Void}, Ptr{Float64}, Ptr{Int32}, Ptr{Int32}, Ref{Int64}, Ref{Int64}, Ref{Int64}),
                         ctx.ptr, xyz, count, cell, m, n_in, dropped), "get_voxels")
    ([SVector{3, Float64}(xyz[:, i]) for i in 1:m[]], count, cell, Int(n_in[]), Int(dropped[]))
end

"For every input point the 1-based index of its voxel in the resident cloud, 0 for a dropped point (fsdf_get_voxel_of_point)."
function voxel_of_point(ctx::Context)
    n = Ref{Int64}(0)
    check(ctx.ptr, ccall((:fsdf_get_voxel_of_point, lib), Cint, (Ptr{Void}, Ptr{Int32}, Ref{Int64}),
                         ctx.ptr, C_NULL, n), "get_voxel_of_point")
    out = zeros(Int32, n[])
    check(ctx.ptr, ccall((:fsdf_get_voxel_of_point, lib), Cint, (Ptr{Void}, Ptr{Int32}, Ref{Int64}),
                         ctx.ptr, out, n), "get_voxel_of_point")
    out .+ Int32(1)
end

"One GPU's shard of the frame's cloud (the cost is a sum over points,
src/gradientdescent.jl:32): the whole cloud is Hilbert-sorted on the device and
this context keeps the contiguous range [first, last] (1-based, inclusive) of
that order — the partition of DESIGN.md §6, balanced by fsdf_chunk_costs."
function set_points_range!{T}(ctx::Context, pts::AbstractVector{SVector{3, T}}, first::Integer, last::Integer)
    P = convert(Vector{SVector{3, Float64}}, pts)
    check(ctx.ptr, ccall((:fsdf_set_points_range, lib), Cint, (Ptr{Void}, Ptr{Float64}, Int64, Int64, Int64),
                         ctx.ptr, reinterpret(Float64, P), length(P), first - 1, last), "set_points_range")
end

"Once per frame, after its first cost evaluation: regroup the resident cloud by
each point's nearest surface in that pass (fsdf_regroup_points). The frame's
later evaluations (the rest of track!'s iterations, src/tracking.jl:8-27) give
the same per-point results and evaluate fewer hulls per 64-point chunk."
regroup_points!(ctx::Context) = check(ctx.ptr, ccall((:fsdf_regroup_points, lib), Cint, (Ptr{Void},), ctx.ptr),
                                      "regroup_points")

"The same where the library's rule says it pays (fsdf_regroup_auto: the last pass
ran one wave per 64-point chunk — clouds above the planned window); true when it
regrouped. GPUCost applies it after a new cloud's first evaluation."
function regroup_auto!(ctx::Context)
    applied = Ref{Int32}(0)
    check(ctx.ptr, ccall((:fsdf_regroup_auto, lib), Cint, (Ptr{Void}, Ref{Int32}), ctx.ptr, applied), "regroup_auto")
    applied[] != 0
end

"The posed scene in the state's number type (Float64 or Dual): per surface the
world pose (R, t) (identity for RBF skins) and, per RBF skin, its world centres
and solved coefficients u = (w; a; b)."
immutable SceneGeometry{T}
    R::Vector{Matrix{T}}
    t::Vector{Vector{T}}
    centres::Vector{Vector{SVector{3, T}}}
    u::Vector{Vector{T}}
end

function scene_geometry{P, T}(state::ManipulatorState{P, T, T})
    R = Matrix{T}[]; t = Vector{T}[]; C = Vector{SVector{3, T}}[]; U = Vector{T}[]
    o = SVector{3, Float64}(0, 0, 0)
    for s in state.manipulator.surfaces
        if isa(s, ConvexGeometry)
            A = convert(AffineMap, transform_to_root(state.mechanism_state, s.frame))   # src/Flash.jl:248
            push!(R, Matrix{T}(transform_deriv(A, o)))
            push!(t, Vector{T}(A(o)))
        else
            push!(R, eye(T, 3)); push!(t, zeros(T, 3))
            # src/Flash.jl:207-212: surface points (value 0, deformed) and skeleton points (value −1)
            sp = Flash.surface_points(state, s)
            kp = Flash.skeleton_points(state, s)
            c = vcat(sp, kp)
            n = length(c)
            M = zeros(T, n + 4, n + 4)   # [A P; Pᵀ 0], A_ij = |c_i − c_j|³ (XCubed), P_i = [1 c_iᵀ]
            for i in 1:n, j in 1:n
                M[i, j] = i == j ? zero(T) : norm(c[i] - c[j])^3
            end
            for i in 1:n
                M[i, n + 1] = M[n + 1, i] = one(T)
                for d in 1:3
                    M[i, n + 1 + d] = M[n + 1 + d, i] = c[i][d]
                end
            end
            rhs = vcat(zeros(T, length(sp)), -ones(T, length(kp)), zeros(T, 4))
            push!(C, c)
            push!(U, M \ rhs)
        end
    end
    SceneGeometry{T}(R, t, C, U)
end

"(poses [12 × S] row-major R then t; RBF rows [4 × Σ(n+1)]: (c_i, w_i) then (a, b))."
function device_inputs(geo::SceneGeometry)
    S = length(geo.R)
    poses = zeros(12, S)
    for k in 1:S
        R = map(value, geo.R[k])
        poses[1:9, k] = vec(R')
        poses[10:12, k] = map(value, geo.t[k])
    end
    rows = Float64[]
    for (c, u) in zip(geo.centres, geo.u)
        n = length(c)
        for i in 1:n
            append!(rows, [value(c[i][1]), value(c[i][2]), value(c[i][3]), value(u[i])])
        end
        append!(rows, map(value, u[n + 1:n + 4]))
    end
    poses, rows
end

"Drop-in for CostFunctor(manipulator, sensed_points) (src/gradientdescent.jl:41-57)."
type GPUCost{P} <: Function
    manipulator::Manipulator{P}
    ctx::Context
    states::Dict{DataType, ManipulatorState}   # one per number type, as CostFunctor caches it (:50-53)
    memo_x::Vector{Float64}
    memo_accum::Vector{Float64}
    weight::Float64
    fresh::Bool   # the resident cloud has not been evaluated yet (the regroup follows its first pass)
    robust::Bool  # a loss other than LOSS_SQUARE is set: the pass is fsdf_eval_robust's
end

# fsdf_set_loss kinds (include/flashsdf.h "robust point losses")
const LOSS_SQUARE = Int32(0)
const LOSS_HUBER = Int32(1)
const LOSS_TUKEY = Int32(2)

"""
The robust point loss of the context (fsdf_set_loss): `kind` LOSS_HUBER or LOSS_TUKEY with a
finite `scale` > 0, or LOSS_SQUARE (least squares, the default). Kept over model and cloud swaps.
"""
set_loss!(ctx::Context, kind::Integer, scale::Real) =   # (fsdf_set_loss with the scale by reference)
    check(ctx.ptr, ccall((:fsdf_set_loss_ref, lib), Cint, (Ptr{Void}, Int32, Ptr{Float64}),
                         ctx.ptr, Int32(kind), Float64[scale]), "set_loss")

"(kind, scale) as the library holds them (fsdf_get_loss)."
function get_loss(ctx::Context)
    kind = Ref{Int32}(0); scale = Ref{Float64}(0)
    check(ctx.ptr, ccall((:fsdf_get_loss, lib), Cint, (Ptr{Void}, Ref{Int32}, Ref{Float64}),
                         ctx.ptr, kind, scale), "get_loss")
    kind[], scale[]
end

"""
One residual pass over the resident cloud of a hull-only scene and the per-surface sums of the
context's loss, reduced on the device (fsdf_eval_robust): returns (cost Σρ, accumulator with the
robust wrenches Σ 2 w d* v in fsdf_eval's layout, moments 21 x S of Σ w v vᵀ, weights Σ w per surface).
"""
function eval_robust(ctx::Context, poses::Vector{Float64})
    S = div(length(poses), 12)
    accum = zeros(1 + 6S)
    moments = zeros(21, S)
    weights = zeros(S)
    c = Ref{Float64}(0)
    check(ctx.ptr, ccall((:fsdf_eval_robust, lib), Cint,
                         (Ptr{Void}, Ptr{Float64}, Ref{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}),
                         ctx.ptr, poses, c, accum, moments, weights), "eval_robust")
    c[], accum, moments, weights
end

"""
Serve robust objectives (a loss, point weights, a free-space split) on scenes with RBF skins and
deformations too (fsdf_set_robust_skins; off by default: such scenes are then refused as before).
"""
set_robust_skins!(ctx::Context, enable::Bool) =
    check(ctx.ptr, ccall((:fsdf_set_robust_skins, lib), Cint, (Ptr{Void}, Int32), ctx.ptr, Int32(enable)),
          "set_robust_skins")

"""
eval_robust on a scene with RBF skins (fsdf_eval_robust_skins; needs set_robust_skins!): returns
(cost Σρ, accumulator in fsdf_eval's full layout — a skin's wrench 0, then the skins' robust blocks
Σ 2 (aw d*) j —, moments 21 x S with a skin's column zero, weights Σ aw per surface).
"""
function eval_robust_skins(ctx::Context, poses::Vector{Float64})
    S = div(length(poses), 12)
    accum = zeros(ctx.accum_len)
    moments = zeros(21, S)
    weights = zeros(S)
    c = Ref{Float64}(0)
    check(ctx.ptr, ccall((:fsdf_eval_robust_skins, lib), Cint,
                         (Ptr{Void}, Ptr{Float64}, Ref{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64},
                          Ptr{Float64}),
                         ctx.ptr, poses, c, accum, moments, C_NULL, weights), "eval_robust_skins")
    c[], accum, moments, weights
end

"""
Let a robust objective (a loss, point weights, a free-space split) run on the device-resident solver
loops of fsdf_descend / fsdf_descend_lm (fsdf_set_robust_loops; hull-only rigid scenes, the host
loop's bits). Off by default: such objectives take the host loop and the required modes are refused.
"""
set_robust_loops!(ctx::Context, enable::Bool) =
    check(ctx.ptr, ccall((:fsdf_set_robust_loops, lib), Cint, (Ptr{Void}, Int32), ctx.ptr, Int32(enable)),
          "set_robust_loops")

"The switch as the library holds it (fsdf_get_robust_loops)."
function get_robust_loops(ctx::Context)
    v = Ref{Int32}(0)
    check(ctx.ptr, ccall((:fsdf_get_robust_loops, lib), Cint, (Ptr{Void}, Ref{Int32}), ctx.ptr, v),
          "get_robust_loops")
    v[] != 0
end

"""
eval_robust without its synchronisation and read-back (fsdf_eval_robust_device): the pass, the robust
launch and the rows' assembly are enqueued on the context stream; d_accum (1 + 6S doubles) and
d_moments (21 x S doubles, or C_NULL for none) are device pointers, filled with eval_robust's bits.
"""
eval_robust_device(ctx::Context, poses::Vector{Float64}, d_accum::Ptr{Float64},
                   d_moments::Ptr{Float64}=Ptr{Float64}(C_NULL)) =
    check(ctx.ptr, ccall((:fsdf_eval_robust_device, lib), Cint,
                         (Ptr{Void}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}),
                         ctx.ptr, poses, d_accum, d_moments), "eval_robust_device")

"""
Score B candidate pose sets against the resident cloud in one batch of launches (fsdf_score_poses):
poses is 12 x S x B (each candidate as eval_robust takes it); returns the B costs — eval_robust's
cost at each candidate under the context's loss, weights and split, as a sum, with no gradient.
Hull-only scenes; read-only on the context.
"""
function score_poses(ctx::Context, poses::Array{Float64}, B::Integer)
    cost = zeros(B)
    check(ctx.ptr, ccall((:fsdf_score_poses, lib), Cint, (Ptr{Void}, Ptr{Float64}, Int32, Ptr{Float64}),
                         ctx.ptr, poses, Int32(B), cost), "score_poses")
    cost
end

"""
score_poses from states (fsdf_score_states): x is nq x B; the library runs its own forward
kinematics per candidate, so the context needs a mechanism registered through the C interface
(fsdf_set_mechanism; this shim keeps RigidBodyDynamics and registers none: FSDF_ERR_STATE).
"""
function score_states(ctx::Context, x::Array{Float64}, B::Integer)
    cost = zeros(B)
    check(ctx.ptr, ccall((:fsdf_score_states, lib), Cint, (Ptr{Void}, Ptr{Float64}, Int32, Ptr{Float64}),
                         ctx.ptr, x, Int32(B), cost), "score_states")
    cost
end

"(summed milliseconds of the scoring calls' launches, calls recorded) since the last query (fsdf_score_time)."
function score_time(ctx::Context)
    ms = Ref{Float64}(0)
    n = Ref{Int64}(0)
    check(ctx.ptr, ccall((:fsdf_score_time, lib), Cint, (Ptr{Void}, Ref{Float64}, Ref{Int64}), ctx.ptr, ms, n),
          "score_time")
    ms[], n[]
end

"""
eval_robust at B candidate pose sets in one batch of launches (fsdf_batch_robust_poses): poses is
12 x S x B; returns (accum (1 + 6S) x B, moments 21 x S x B, weights S x B), each candidate's bit
for bit what eval_robust returns at its poses. Hull-only scenes; read-only on the context.
"""
function batch_robust_poses(ctx::Context, poses::Array{Float64}, S::Integer, B::Integer)
    accum = zeros(1 + 6S, B)
    moments = zeros(21, S, B)
    weights = zeros(S, B)
    check(ctx.ptr, ccall((:fsdf_batch_robust_poses, lib), Cint,
                         (Ptr{Void}, Ptr{Float64}, Int32, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}),
                         ctx.ptr, poses, Int32(B), accum, moments, weights), "batch_robust_poses")
    accum, moments, weights
end

"""
(cost, gradient, Gauss-Newton Hessian) at B states in one batch of launches (fsdf_batch_states): x is
nq x B. As score_states, the library runs its own forward kinematics and chain rule, so the context
needs a mechanism registered through the C interface (this shim registers none: FSDF_ERR_STATE).
"""
function batch_states(ctx::Context, x::Array{Float64}, nq::Integer, B::Integer)
    cost = zeros(B)
    grad = zeros(nq, B)
    hess = zeros(nq, nq, B)
    check(ctx.ptr, ccall((:fsdf_batch_states, lib), Cint,
                         (Ptr{Void}, Ptr{Float64}, Int32, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}),
                         ctx.ptr, x, Int32(B), cost, grad, hess), "batch_states")
    cost, grad, hess
end

"""
The Levenberg-Marquardt loop from B starts in lockstep (fsdf_descend_lm_batch_ref: the scalars go by
reference, as set_loss!'s): x (nq x B) is updated in place. Needs a mechanism registered through C,
as batch_states.
"""
function descend_lm_batch!(ctx::Context, x::Array{Float64}, B::Integer, iteration_limit::Integer, damping::Real,
                           max_step::Real, tolerance::Real, n_points::Real)
    params = Float64[damping, max_step, tolerance, n_points]
    value = zeros(B)
    iterations = zeros(Int32, B)
    lambda = zeros(B)
    check(ctx.ptr, ccall((:fsdf_descend_lm_batch_ref, lib), Cint,
                         (Ptr{Void}, Ptr{Float64}, Int32, Int32, Ptr{Float64}, Ptr{Float64}, Ptr{Int32}, Ptr{Float64}),
                         ctx.ptr, x, Int32(B), Int32(iteration_limit), params, value, iterations, lambda),
          "descend_lm_batch")
    value, iterations, lambda
end

"The NaiveSolver loop from B starts in lockstep (fsdf_descend_batch_ref): x (nq x B) is updated in place; divisors nq."
function descend_batch!(ctx::Context, x::Array{Float64}, B::Integer, iteration_limit::Integer, rate::Real,
                        max_step::Real, tolerance::Real, divisors::Vector{Float64}, n_points::Real)
    params = Float64[rate, max_step, tolerance, n_points]
    value = zeros(B)
    iterations = zeros(Int32, B)
    check(ctx.ptr, ccall((:fsdf_descend_batch_ref, lib), Cint,
                         (Ptr{Void}, Ptr{Float64}, Int32, Int32, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Int32}),
                         ctx.ptr, x, Int32(B), Int32(iteration_limit), params, divisors, value, iterations),
          "descend_batch")
    value, iterations
end

"(summed milliseconds of the batched calls' launches, calls recorded) since the last query (fsdf_batch_time)."
function batch_time(ctx::Context)
    ms = Ref{Float64}(0)
    n = Ref{Int64}(0)
    check(ctx.ptr, ccall((:fsdf_batch_time, lib), Cint, (Ptr{Void}, Ref{Float64}, Ref{Int64}), ctx.ptr, ms, n),
          "batch_time")
    ms[], n[]
end

"""
Per-point confidence weights a_i >= 0 (finite) of the resident cloud, in the order of the points
given to set_points! (fsdf_set_point_weights): every sum of eval_robust carries a_i as a factor
of point i's terms (cost Σ a ρ, wrench Σ 2 a w d* v, moments Σ a w v vᵀ). They belong to the
resident cloud: every set_points! clears them. Hull-only scenes.
"""
set_point_weights!(ctx::Context, weights::Vector{Float64}) =
    check(ctx.ptr, ccall((:fsdf_set_point_weights, lib), Cint, (Ptr{Void}, Ptr{Float64}, Int64),
                         ctx.ptr, weights, length(weights)), "set_point_weights")

"Every point counts 1 again (fsdf_set_point_weights with NULL)."
clear_point_weights!(ctx::Context) =
    check(ctx.ptr, ccall((:fsdf_set_point_weights, lib), Cint, (Ptr{Void}, Ptr{Float64}, Int64),
                         ctx.ptr, C_NULL, 0), "set_point_weights")

"The weights of the `n` resident points in resident order, or `nothing` when none are set (fsdf_get_point_weights)."
function point_weights(ctx::Context, n::Integer)
    set = Ref{Int32}(0)
    out = zeros(n)
    check(ctx.ptr, ccall((:fsdf_get_point_weights, lib), Cint, (Ptr{Void}, Ptr{Float64}, Ref{Int32}),
                         ctx.ptr, out, set), "get_point_weights")
    set[] != 0 ? out : nothing
end

"Weights for a GPUCost's sensed points: its passes then go through fsdf_eval_robust (hull-only scenes)."
function set_point_weights!(f::GPUCost, weights::Vector{Float64})
    set_point_weights!(f.ctx, weights)
    f.robust = true
    f.memo_x = Float64[]   # (another objective: the memoised pass no longer holds)
    f
end

"`loss = (kind, scale)`: a robust point loss in place of the squared distance (hull-only scenes)."
function GPUCost(manipulator::Manipulator, sensed_points::AbstractVector;
                 device::Integer=0, deformation_cost_weight=default_deformation_cost_weight,
                 loss::Tuple=(LOSS_SQUARE, 0.0))
    ctx = Context(manipulator; device=device)
    set_points!(ctx, sensed_points)
    set_loss!(ctx, loss[1], loss[2])
    GPUCost(manipulator, ctx, Dict{DataType, ManipulatorState}(), Float64[], Float64[],
            Float64(deformation_cost_weight), true, loss[1] != LOSS_SQUARE)
end

function state_for{T}(f::GPUCost, ::Type{T})
    get!(f.states, T) do
        ManipulatorState(f.manipulator, T, T)
    end
end

"One residual pass per distinct value(x): cost Σ d² (with a loss: Σ ρ(d)) and the accumulator."
function residual_pass!(f::GPUCost, geo::SceneGeometry, xv::Vector{Float64})
    if xv != f.memo_x
        poses, rows = device_inputs(geo)
        if !isempty(rows)
            check(f.ctx.ptr, ccall((:fsdf_set_rbf_params, lib), Cint, (Ptr{Void}, Ptr{Float64}, Int64),
                                   f.ctx.ptr, rows, length(rows)), "set_rbf_params")
        end
        accum = zeros(f.ctx.accum_len)   # 1 + 6S + Σ(4n+4) (fsdf_accum_len)
        c = Ref{Float64}(0)
        if f.robust   # Σρ and the robust wrenches, in the same accumulator layout (hull-only scenes)
            check(f.ctx.ptr, ccall((:fsdf_eval_robust, lib), Cint,
                                   (Ptr{Void}, Ptr{Float64}, Ref{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}),
                                   f.ctx.ptr, poses, c, accum, C_NULL, C_NULL), "eval_robust")
        else
            check(f.ctx.ptr, ccall((:fsdf_eval, lib), Cint,
                                   (Ptr{Void}, Ptr{Float64}, Ref{Float64}, Ptr{Float64}, Ptr{Int32}, Ptr{Float64},
                                    Ptr{Float64}),
                                   f.ctx.ptr, poses, c, accum, C_NULL, C_NULL, C_NULL), "eval")
        end
        if f.fresh   # once per frame, after its first pass (per-point results unchanged, sums to rounding)
            regroup_auto!(f.ctx)
            f.fresh = false
        end
        f.memo_x = copy(xv)
        f.memo_accum = accum
    end
    f.memo_accum
end

"""
One residual pass over the resident cloud of a rigid scene (poses as `device_inputs`
returns them) with the per-surface second moments of its residual, reduced on the device
(fsdf_eval_moments): returns (cost, accumulator, moments 21 x S — per surface the upper
triangle, row-major, of Σ w wᵀ with w = (∇d*, p × ∇d*)), the input of a Gauss-Newton
Hessian (fsdf_gauss_newton_matrix).
"""
function eval_moments(ctx::Context, poses::Vector{Float64})
    accum = zeros(ctx.accum_len)
    moments = zeros(21, div(length(poses), 12))
    c = Ref{Float64}(0)
    check(ctx.ptr, ccall((:fsdf_eval_moments, lib), Cint,
                         (Ptr{Void}, Ptr{Float64}, Ref{Float64}, Ptr{Float64}, Ptr{Float64}),
                         ctx.ptr, poses, c, accum, moments), "eval_moments")
    c[], accum, moments
end

"""
The prior of fsdf_descend_lm on the frame's start state (fsdf_set_lm_prior): its
objective becomes c/N + Σ weight[i] (x[i] − x̄[i])², x̄ the x handed to that call; one
weight >= 0 per joint coordinate, quaternion coordinates penalised raw. An empty vector
clears it.
"""
set_lm_prior!(ctx::Context, weight::Vector{Float64}) =
    check(ctx.ptr, ccall((:fsdf_set_lm_prior, lib), Cint, (Ptr{Void}, Ptr{Float64}, Int32),
                         ctx.ptr, weight, Int32(length(weight))), "set_lm_prior")

"""
Where fsdf_descend_lm's loop runs (fsdf_set_lm_solver): 0 the host loop (default), 1 the
device loop where the scene fits, 2 the device loop required. The same bits.
"""
set_lm_solver!(ctx::Context, mode::Integer) =
    check(ctx.ptr, ccall((:fsdf_set_lm_solver, lib), Cint, (Ptr{Void}, Int32), ctx.ptr, Int32(mode)),
          "set_lm_solver")

# Σ_p d*(p)² as a number of the state's type: the value from the pass; for a
# Dual chunk, the first-order change of the cost through every surface pose
# (δc = −(ω·(M − t×F) + δt·F) with ω = vee(δR Rᵀ)) and every RBF skin's
# centres and coefficients (δc = Σ E_i·δc_i + λ·δu).
assemble(geo::SceneGeometry{Float64}, accum::Vector{Float64}) = accum[1]

function assemble{N, V}(geo::SceneGeometry{Dual{N, V}}, accum::Vector{Float64})
    g = zeros(N)
    S = length(geo.R)
    for k in 1:S
        F = accum[2 + 6(k - 1):4 + 6(k - 1)]
        M = accum[5 + 6(k - 1):7 + 6(k - 1)]
        Rk = geo.R[k]; tk = geo.t[k]
        Rv = map(value, Rk); tv = map(value, tk)
        Mo = M - cross(tv, F)
        for p in 1:N
            dR = Float64[partials(Rk[i, j], p) for i in 1:3, j in 1:3]
            W = dR * Rv'
            ω = 0.5 * [W[3, 2] - W[2, 3], W[1, 3] - W[3, 1], W[2, 1] - W[1, 2]]
            dt = Float64[partials(tk[i], p) for i in 1:3]
            g[p] -= dot(ω, Mo) + dot(dt, F)
        end
    end
    off = 2 + 6S
    for (c, u) in zip(geo.centres, geo.u)
        n = length(c)
        lam = accum[off:off + n + 3]             # λ_w (n), λ_a, λ_b (3)
        E = accum[off + n + 4:off + 4n + 3]      # E_i (3 each)
        off += 4n + 4
        for p in 1:N
            s = 0.0
            for i in 1:n, d in 1:3
                s += E[3(i - 1) + d] * partials(c[i][d], p)
            end
            for i in 1:n + 4
                s += lam[i] * partials(u[i], p)
            end
            g[p] += s
        end
    end
    Dual(accum[1], ForwardDiff.Partials(tuple(g...)))
end

function (f::GPUCost){T}(x::AbstractVector{T})
    state = state_for(f, T)
    unflatten!(state, x)
    normalize!(state.mechanism_state)   # src/gradientdescent.jl:30 — in T, so its projection reaches the partials
    geo = scene_geometry(state)
    accum = residual_pass!(f, geo, Float64[value(xi) for xi in x])
    c = assemble(geo, accum)
    for deformation_set in values(state.deformations)   # src/gradientdescent.jl:33-37
        for deformation in deformation_set
            c += f.weight * sum(deformation .^ 2)
        end
    end
    c
end

"Flash.skin(state) (src/Flash.jl:265-268) on the device: x -> minimum over surfaces."
function skin(ctx::Context, state::ManipulatorState)
    poses, rows = device_inputs(scene_geometry(state))
    if !isempty(rows)
        check(ctx.ptr, ccall((:fsdf_set_rbf_params, lib), Cint, (Ptr{Void}, Ptr{Float64}, Int64),
                             ctx.ptr, rows, length(rows)), "set_rbf_params")
    end
    function (x)
        d = Ref{Float64}(0); k = Ref{Int32}(0); g = zeros(3)
        xyz = Float64[x[1], x[2], x[3]]
        check(ctx.ptr, ccall((:fsdf_skin, lib), Cint,
                             (Ptr{Void}, Ptr{Float64}, Ptr{Float64}, Int64, Ptr{Float64}, Ptr{Int32}, Ptr{Float64}),
                             ctx.ptr, poses, xyz, 1, d, k, g), "skin")
        d[]
    end
end

end # module
