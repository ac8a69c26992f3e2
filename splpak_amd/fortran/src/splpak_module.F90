!> Drop-in `splpak_module` for MI355X: the public surface of jacobwilliams/splpak
!! (`splpak_wp`, `splpak_type` with the generics `initialize` => splcc/splcw,
!! `evaluate` => splfe/splde and `destroy`; reference src/splpak.F90:43-127) over the
!! HIP library `libsplpak_hip.so` (C ABI in include/splpak_hip.h).
!!
!! Argument lists, `ierror` codes and the text printed on `output_unit` follow the
!! reference (splcw :512-513, splcc :421-422, splde :1089, splfe :1258, cfaerr :399-407).
!! The fit and every batched evaluation run on the GPU and never fall back: without a GPU those calls
!! fail with a negative `ierror` and the library's message is printed.  A separate HOST solver
!! (splpak_host.F90, written from scratch for this package) runs only when the caller selects it
!! explicitly with `call solver%set_host(.true.)`, and in a -DREAL128 build (no GPU arithmetic).  The SCALAR
!! `evaluate` (one point per call, the reference's splfe/splde) is computed on the host by this
!! module itself (SURVEY 7.2 H6: one kernel launch per point would cost 10^4 x its arithmetic);
!! `evaluate_many` is the GPU path.
!!
!! Differences a caller can observe (documented in INTEGRATION.md):
!!  * `work` is not used as scratch.  The reference's 106 check on `nwrk` is kept; the
!!    larger requirement of the dense solver (error 107 via suprls 32, :1443-1454) is
!!    not enforced, because the GPU path does not need the ncol*(ncol+1) array (550 GB
!!    at 64^3 nodes).  After a successful fit with xtrap /= 0 `work(1:ncol)` holds the
!!    sparse-area histogram exactly as the reference leaves it (:879-907).
!!  * additive: `evaluate_many` evaluates a batch of points in one kernel launch,
!!    `evaluate_derivatives` value + gradient (+ Hessian) of a batch in one pass,
!!    `refit` fits new values on the points of the last `initialize` with the factorisation that fit left on the GPU,
!!    `evaluate_fields` evaluates several coefficient sets (what `refit` returns) at the same batch of points in one call,
!!    `evaluate_each` evaluates the fits of `initialize_many`, each at its own points, and `residuals_each` forms their residuals
!!    and per-problem sums, one launch each,
!!    `initialize_many_clipped` runs the sigma-clipping loop of those two around `initialize_many` inside the one launch,
!!    `initialize_many_robust` is that loop on a median / MAD scale with returning points, and `mad_each` its selection alone,
!!    `initialize_many_cov` is `initialize_many` with the covariance of the coefficients, and `variance_each` the prediction
!!    variance of those fits, each at its own points,
!!    `evaluate_grid` evaluates every point of a tensor-product grid of points from its axes alone,
!!    `evaluate_grid_derivatives` value + gradient (+ Hessian) on such a grid, one plane per entry, in one pass,
!!    `integrate_grid` integrates the fit over the cells of a tensor grid (cell integrals, projections), `integrate` over one box,
!!    `last_fit_info` returns the diagnostics of the last fit (the residual norm `reserr` that the
!!    reference computes, suprls :1693, and drops, splcw :690; row counts; refinement steps).
!!
!! Build with -DREAL32 for single precision storage (as the reference, :33-41); -DREAL128 builds the
!! module on the host solver alone (quad precision has no MI355X arithmetic).
module splpak_module

    use iso_c_binding
    use iso_fortran_env, only: real32, real64, real128, output_unit
    use splpak_host_solver, only: hk, host_basis, host_fit

    implicit none

    private

#ifdef REAL32
    integer,parameter :: wp = real32
#elif REAL128
    integer,parameter :: wp = real128
#else
    integer,parameter :: wp = real64
#endif

    integer,parameter,public :: splpak_wp = wp   !! working precision

    integer,save :: no_gpu_optin = -1            !! SPLPAK_HOST_IF_NO_GPU as read once (-1: not read yet)
    logical,save :: no_gpu_said = .false.        !! the one line about it has been printed

    type,public :: splpak_type
        private
        integer :: mdim = 0    !! dimension of the last call (the reference keeps scratch here, :95-111)
        real(real64) :: info(10) = 0.0_real64   !! diagnostics of the last fit (include/splpak_hip.h, `info`)
        integer :: ngpus = 1   !! GPUs of this node the fit is spread over (set_gpus)
        integer(c_int64_t) :: token = 0       !! of the last successful single-GPU `initialize` (splpak_fit_token; 0: nothing to refit)
        integer(c_int64_t) :: fit_ndata = 0   !! its points
        integer(c_int64_t) :: fit_ncol = 0    !! its coefficients
        logical :: fit_fell_to_host = .false. !! the last `initialize` ran on the host for want of a GPU (SPLPAK_HOST_IF_NO_GPU)
#ifdef REAL128
        logical :: host = .true.    !! quad precision: the host solver is the only path
#else
        logical :: host = .false.   !! .true. after set_host(.true.): fits and batches run on the host solver (never a fallback)
#endif
    contains
        private
        generic,public   :: initialize    => splcc, splcw        !! fit
        procedure,public :: initialize_grid => splpak_fit_grid      !! fit of samples on a tensor-product grid of points (additive)
        procedure,public :: initialize_grid_weighted => splpak_fit_grid_weighted   !! the same with a weight per sample (additive)
        procedure,public :: initialize_many => splpak_fit_many      !! many small independent fits on one node grid in one launch (additive)
        procedure,public :: initialize_many_clipped => splpak_fit_many_clipped !! .. with sigma clipping, the loop in the same launch (additive)
        procedure,public :: initialize_many_cov => splpak_fit_many_cov !! initialize_many with the covariance of the coefficients (additive)
        procedure,public :: variance_each => splpak_variance_each !! the prediction variance of those fits, each at its own points (additive)
        procedure,public :: evaluate_each => splpak_eval_each      !! the fits of initialize_many, each at its own points, in one launch (additive)
        procedure,public :: initialize_many_robust => splpak_fit_many_robust !! .. clipped on a median / MAD scale, points may return (additive)
        procedure,public :: mad_each => splpak_mad_each !! the median and the MAD of every problem's values in one launch (additive)
        procedure,public :: residuals_each => splpak_residuals_each !! their residuals and per-problem sums in one launch (additive)
        generic,public   :: evaluate      => splfe, splde        !! one point
        generic,public   :: evaluate_many => splfe_many, splde_many  !! batch of points (additive)
        procedure,public :: evaluate_derivatives => splpak_derivs_many !! value + gradient (+ Hessian) of a batch (additive)
        procedure,public :: evaluate_grid => splpak_eval_grid       !! every point of a tensor-product grid of points (additive)
        procedure,public :: evaluate_grid_derivatives => splpak_eval_grid_derivs !! value + gradient (+ Hessian) planes on such a grid (additive)
        procedure,public :: integrate_grid => splpak_integrate_grid !! integrals over the cells of a tensor grid, projections (additive)
        procedure,public :: integrate     => splpak_integrate       !! the integral over one box (additive)
        procedure,public :: evaluate_fields => splpak_eval_fields   !! several coefficient sets at the same batch of points (additive)
        procedure,public :: refit         => splpak_refit           !! new values on the points of the last `initialize` (additive)
        procedure,public :: destroy       => destroy_splpak
        procedure,public :: last_fit_info => splpak_last_fit_info   !! reserr, row counts, ... of the last fit (additive)
        procedure,public,nopass :: set_option => splpak_set_option    !! a named option of the HIP library for the following fits (additive)
        procedure,public :: set_gpus      => splpak_set_gpus        !! spread the following fits over n GPUs of this node (additive)
        procedure,public :: set_host      => splpak_set_host        !! run the following calls on the host solver (additive; explicit, never a fallback)
        procedure,private :: splcc
        procedure,private :: splcw
        procedure,private :: splfe
        procedure,private :: splde
        procedure,private :: splfe_many
        procedure,private :: splde_many
        procedure,private :: splpak_derivs_many
        procedure,private :: splpak_eval_grid
        procedure,private :: splpak_eval_grid_derivs
        procedure,private :: splpak_eval_fields
        procedure,private :: splpak_integrate_grid
        procedure,private :: splpak_integrate
    end type splpak_type

#ifndef REAL128
    interface
#ifdef REAL32
        integer(c_int32_t) function c_fit(ndim,xdata,l1xdat,ydata,wdata,ndata,xmin,xmax,nodes,xtrap,&
                                          coef,ncf,nwrk,hist,info) bind(C,name='splpak_fit_f32')
#else
        integer(c_int32_t) function c_fit(ndim,xdata,l1xdat,ydata,wdata,ndata,xmin,xmax,nodes,xtrap,&
                                          coef,ncf,nwrk,hist,info) bind(C,name='splpak_fit_f64')
#endif
            import :: c_int32_t, c_int64_t, c_ptr, wp
            integer(c_int32_t),value :: ndim, l1xdat
            integer(c_int64_t),value :: ndata, ncf, nwrk
            type(c_ptr),value :: xdata, ydata, wdata, xmin, xmax, nodes, coef, hist, info
            real(wp),value :: xtrap
        end function c_fit
#ifdef REAL32
        integer(c_int32_t) function c_eval(ndim,nq,xq,ldxq,nderiv,coef,xmin,xmax,nodes,out) &
                                           bind(C,name='splpak_eval_f32')
#else
        integer(c_int32_t) function c_eval(ndim,nq,xq,ldxq,nderiv,coef,xmin,xmax,nodes,out) &
                                           bind(C,name='splpak_eval_f64')
#endif
            import :: c_int32_t, c_int64_t, c_ptr
            integer(c_int32_t),value :: ndim, ldxq
            integer(c_int64_t),value :: nq
            type(c_ptr),value :: xq, nderiv, coef, xmin, xmax, nodes, out
        end function c_eval
#ifdef REAL32
        integer(c_int32_t) function c_eval_derivs(ndim,nq,xq,ldxq,order,coef,xmin,xmax,nodes,out,ldout) &
                                                  bind(C,name='splpak_eval_derivs_f32')
#else
        integer(c_int32_t) function c_eval_derivs(ndim,nq,xq,ldxq,order,coef,xmin,xmax,nodes,out,ldout) &
                                                  bind(C,name='splpak_eval_derivs_f64')
#endif
            import :: c_int32_t, c_int64_t, c_ptr
            integer(c_int32_t),value :: ndim, ldxq, order, ldout
            integer(c_int64_t),value :: nq
            type(c_ptr),value :: xq, coef, xmin, xmax, nodes, out
        end function c_eval_derivs
#ifdef REAL32
        integer(c_int32_t) function c_eval_grid(ndim,npts,axes,nderiv,coef,xmin,xmax,nodes,out) &
                                                bind(C,name='splpak_eval_grid_f32')
#else
        integer(c_int32_t) function c_eval_grid(ndim,npts,axes,nderiv,coef,xmin,xmax,nodes,out) &
                                                bind(C,name='splpak_eval_grid_f64')
#endif
            import :: c_int32_t, c_ptr
            integer(c_int32_t),value :: ndim
            type(c_ptr),value :: npts, axes, nderiv, coef, xmin, xmax, nodes, out
        end function c_eval_grid
#ifdef REAL32
        integer(c_int32_t) function c_eval_grid_derivs(ndim,npts,axes,order,coef,xmin,xmax,nodes,out,ldout) &
                                                       bind(C,name='splpak_eval_grid_derivs_f32')
#else
        integer(c_int32_t) function c_eval_grid_derivs(ndim,npts,axes,order,coef,xmin,xmax,nodes,out,ldout) &
                                                       bind(C,name='splpak_eval_grid_derivs_f64')
#endif
            import :: c_int32_t, c_int64_t, c_ptr
            integer(c_int32_t),value :: ndim, order
            integer(c_int64_t),value :: ldout
            type(c_ptr),value :: npts, axes, coef, xmin, xmax, nodes, out
        end function c_eval_grid_derivs
#ifdef REAL32
        integer(c_int32_t) function c_integrate_grid(ndim,ncell,mode,axes,coef,xmin,xmax,nodes,out) &
                                                     bind(C,name='splpak_integrate_grid_f32')
#else
        integer(c_int32_t) function c_integrate_grid(ndim,ncell,mode,axes,coef,xmin,xmax,nodes,out) &
                                                     bind(C,name='splpak_integrate_grid_f64')
#endif
            import :: c_int32_t, c_ptr
            integer(c_int32_t),value :: ndim
            type(c_ptr),value :: ncell, mode, axes, coef, xmin, xmax, nodes, out
        end function c_integrate_grid
#ifdef REAL32
        integer(c_int32_t) function c_fit_grid(ndim,npts,axes,waxes,nfields,values,ldv,xmin,xmax,nodes,xtrap,coef,ldcoef,info) &
                                               bind(C,name='splpak_fit_grid_f32')
#else
        integer(c_int32_t) function c_fit_grid(ndim,npts,axes,waxes,nfields,values,ldv,xmin,xmax,nodes,xtrap,coef,ldcoef,info) &
                                               bind(C,name='splpak_fit_grid_f64')
#endif
            import :: c_int32_t, c_int64_t, c_ptr, wp
            integer(c_int32_t),value :: ndim, nfields
            integer(c_int64_t),value :: ldv, ldcoef
            type(c_ptr),value :: npts, axes, waxes, values, xmin, xmax, nodes, coef, info
            real(wp),value :: xtrap
        end function c_fit_grid
#ifdef REAL32
        integer(c_int32_t) function c_fit_grid_weighted(ndim,npts,axes,nfields,values,ldv,weights,ldw,xmin,xmax,nodes,xtrap,coef, &
                                                        ldcoef,info) bind(C,name='splpak_fit_grid_weighted_f32')
#else
        integer(c_int32_t) function c_fit_grid_weighted(ndim,npts,axes,nfields,values,ldv,weights,ldw,xmin,xmax,nodes,xtrap,coef, &
                                                        ldcoef,info) bind(C,name='splpak_fit_grid_weighted_f64')
#endif
            import :: c_int32_t, c_int64_t, c_ptr, wp
            integer(c_int32_t),value :: ndim, nfields
            integer(c_int64_t),value :: ldv, ldw, ldcoef
            type(c_ptr),value :: npts, axes, values, weights, xmin, xmax, nodes, coef, info
            real(wp),value :: xtrap
        end function c_fit_grid_weighted
#ifdef REAL32
        integer(c_int32_t) function c_fit_many(ndim,nbatch,offsets,xdata,l1xdat,ydata,wdata,xmin,xmax,nodes,xtrap,coef,ldcoef, &
                                               status,info) bind(C,name='splpak_fit_many_f32')
#else
        integer(c_int32_t) function c_fit_many(ndim,nbatch,offsets,xdata,l1xdat,ydata,wdata,xmin,xmax,nodes,xtrap,coef,ldcoef, &
                                               status,info) bind(C,name='splpak_fit_many_f64')
#endif
            import :: c_int32_t, c_int64_t, c_ptr, wp
            integer(c_int32_t),value :: ndim, nbatch, l1xdat
            integer(c_int64_t),value :: ldcoef
            type(c_ptr),value :: offsets, xdata, ydata, wdata, xmin, xmax, nodes, coef, status, info
            real(wp),value :: xtrap
        end function c_fit_many
#ifdef REAL32
        integer(c_int32_t) function c_fit_many_clip(ndim,nbatch,offsets,xdata,l1xdat,ydata,wdata,xmin,xmax,nodes,xtrap,klo,khi, &
                                                    maxpass,wout,coef,ldcoef,status,info,clip) bind(C,name='splpak_fit_many_clip_f32')
#else
        integer(c_int32_t) function c_fit_many_clip(ndim,nbatch,offsets,xdata,l1xdat,ydata,wdata,xmin,xmax,nodes,xtrap,klo,khi, &
                                                    maxpass,wout,coef,ldcoef,status,info,clip) bind(C,name='splpak_fit_many_clip_f64')
#endif
            import :: c_int32_t, c_int64_t, c_ptr, wp
            integer(c_int32_t),value :: ndim, nbatch, l1xdat, maxpass
            integer(c_int64_t),value :: ldcoef
            type(c_ptr),value :: offsets, xdata, ydata, wdata, xmin, xmax, nodes, wout, coef, status, info, clip
            real(wp),value :: xtrap, klo, khi
        end function c_fit_many_clip
#ifdef REAL32
        integer(c_int32_t) function c_fit_many_clip_mad(ndim,nbatch,offsets,xdata,l1xdat,ydata,wdata,xmin,xmax,nodes,xtrap,klo,khi, &
                                                        maxpass,regrow,wout,coef,ldcoef,status,info,clip) &
                                                        bind(C,name='splpak_fit_many_clip_mad_f32')
#else
        integer(c_int32_t) function c_fit_many_clip_mad(ndim,nbatch,offsets,xdata,l1xdat,ydata,wdata,xmin,xmax,nodes,xtrap,klo,khi, &
                                                        maxpass,regrow,wout,coef,ldcoef,status,info,clip) &
                                                        bind(C,name='splpak_fit_many_clip_mad_f64')
#endif
            import :: c_int32_t, c_int64_t, c_ptr, wp
            integer(c_int32_t),value :: ndim, nbatch, l1xdat, maxpass, regrow
            integer(c_int64_t),value :: ldcoef
            type(c_ptr),value :: offsets, xdata, ydata, wdata, xmin, xmax, nodes, wout, coef, status, info, clip
            real(wp),value :: xtrap, klo, khi
        end function c_fit_many_clip_mad
#ifdef REAL32
        integer(c_int32_t) function c_mad_many(nbatch,offsets,values,wsel,stats) bind(C,name='splpak_mad_many_f32')
#else
        integer(c_int32_t) function c_mad_many(nbatch,offsets,values,wsel,stats) bind(C,name='splpak_mad_many_f64')
#endif
            import :: c_int32_t, c_ptr
            integer(c_int32_t),value :: nbatch
            type(c_ptr),value :: offsets, values, wsel, stats
        end function c_mad_many
#ifdef REAL32
        integer(c_int32_t) function c_eval_many(ndim,nbatch,offsets,xq,ldxq,nderiv,coef,ldcoef,xmin,xmax,nodes,out) &
                                                bind(C,name='splpak_eval_many_f32')
#else
        integer(c_int32_t) function c_eval_many(ndim,nbatch,offsets,xq,ldxq,nderiv,coef,ldcoef,xmin,xmax,nodes,out) &
                                                bind(C,name='splpak_eval_many_f64')
#endif
            import :: c_int32_t, c_int64_t, c_ptr
            integer(c_int32_t),value :: ndim, nbatch, ldxq
            integer(c_int64_t),value :: ldcoef
            type(c_ptr),value :: offsets, xq, nderiv, coef, xmin, xmax, nodes, out
        end function c_eval_many
#ifdef REAL32
        integer(c_int32_t) function c_fit_many_cov(ndim,nbatch,offsets,xdata,l1xdat,ydata,wdata,xmin,xmax,nodes,xtrap,coef,ldcoef, &
                                                   cov,ldcov,status,info) bind(C,name='splpak_fit_many_cov_f32')
#else
        integer(c_int32_t) function c_fit_many_cov(ndim,nbatch,offsets,xdata,l1xdat,ydata,wdata,xmin,xmax,nodes,xtrap,coef,ldcoef, &
                                                   cov,ldcov,status,info) bind(C,name='splpak_fit_many_cov_f64')
#endif
            import :: c_int32_t, c_int64_t, c_ptr, wp
            integer(c_int32_t),value :: ndim, nbatch, l1xdat
            integer(c_int64_t),value :: ldcoef, ldcov
            type(c_ptr),value :: offsets, xdata, ydata, wdata, xmin, xmax, nodes, coef, cov, status, info
            real(wp),value :: xtrap
        end function c_fit_many_cov
#ifdef REAL32
        integer(c_int32_t) function c_eval_many_var(ndim,nbatch,offsets,xq,ldxq,nderiv,cov,ldcov,xmin,xmax,nodes,out) &
                                                    bind(C,name='splpak_eval_many_var_f32')
#else
        integer(c_int32_t) function c_eval_many_var(ndim,nbatch,offsets,xq,ldxq,nderiv,cov,ldcov,xmin,xmax,nodes,out) &
                                                    bind(C,name='splpak_eval_many_var_f64')
#endif
            import :: c_int32_t, c_int64_t, c_ptr
            integer(c_int32_t),value :: ndim, nbatch, ldxq
            integer(c_int64_t),value :: ldcov
            type(c_ptr),value :: offsets, xq, nderiv, cov, xmin, xmax, nodes, out
        end function c_eval_many_var
#ifdef REAL32
        integer(c_int32_t) function c_residuals_many(ndim,nbatch,offsets,xdata,l1xdat,ydata,wdata,coef,ldcoef,xmin,xmax,nodes, &
                                                     resid,stats) bind(C,name='splpak_residuals_many_f32')
#else
        integer(c_int32_t) function c_residuals_many(ndim,nbatch,offsets,xdata,l1xdat,ydata,wdata,coef,ldcoef,xmin,xmax,nodes, &
                                                     resid,stats) bind(C,name='splpak_residuals_many_f64')
#endif
            import :: c_int32_t, c_int64_t, c_ptr
            integer(c_int32_t),value :: ndim, nbatch, l1xdat
            integer(c_int64_t),value :: ldcoef
            type(c_ptr),value :: offsets, xdata, ydata, wdata, coef, xmin, xmax, nodes, resid, stats
        end function c_residuals_many
#ifdef REAL32
        integer(c_int32_t) function c_eval_fields(ndim,nq,xq,ldxq,nderiv,nfields,coef,ldcoef,xmin,xmax,nodes,out,ldout) &
                                                  bind(C,name='splpak_eval_fields_f32')
#else
        integer(c_int32_t) function c_eval_fields(ndim,nq,xq,ldxq,nderiv,nfields,coef,ldcoef,xmin,xmax,nodes,out,ldout) &
                                                  bind(C,name='splpak_eval_fields_f64')
#endif
            import :: c_int32_t, c_int64_t, c_ptr
            integer(c_int32_t),value :: ndim, ldxq, nfields
            integer(c_int64_t),value :: nq, ldcoef, ldout
            type(c_ptr),value :: xq, nderiv, coef, xmin, xmax, nodes, out
        end function c_eval_fields
#ifndef REAL32
        integer(c_int32_t) function c_fit_multi(ngpus,ndim,xdata,l1xdat,ydata,wdata,ndata,xmin,xmax,nodes,xtrap,&
                                                coef,ncf,nwrk,hist,info) bind(C,name='splpak_fit_multi_f64')
            import :: c_int32_t, c_int64_t, c_ptr, wp
            integer(c_int32_t),value :: ngpus, ndim, l1xdat
            integer(c_int64_t),value :: ndata, ncf, nwrk
            type(c_ptr),value :: xdata, ydata, wdata, xmin, xmax, nodes, coef, hist, info
            real(wp),value :: xtrap
        end function c_fit_multi
#endif
        integer(c_int64_t) function c_fit_token() bind(C,name='splpak_fit_token')
            import :: c_int64_t
        end function c_fit_token
#ifdef REAL32
        integer(c_int32_t) function c_refit(token,nfields,ydata,ldy,ndata,coef,ldcoef,info) bind(C,name='splpak_refit_f32')
#else
        integer(c_int32_t) function c_refit(token,nfields,ydata,ldy,ndata,coef,ldcoef,info) bind(C,name='splpak_refit_f64')
#endif
            import :: c_int32_t, c_int64_t, c_ptr
            integer(c_int64_t),value :: token, ldy, ndata, ldcoef
            integer(c_int32_t),value :: nfields
            type(c_ptr),value :: ydata, coef, info
        end function c_refit
        subroutine c_shutdown() bind(C,name='splpak_shutdown')
        end subroutine c_shutdown
        integer(c_int32_t) function c_set_default_option(name,val) bind(C,name='splpak_set_default_option')
            import :: c_int32_t, c_char
            character(kind=c_char) :: name(*), val(*)
        end function c_set_default_option
        integer(c_int32_t) function c_last_error(buf,buflen) bind(C,name='splpak_last_error_message')
            import :: c_int32_t, c_char
            character(kind=c_char) :: buf(*)
            integer(c_int32_t),value :: buflen
        end function c_last_error
    end interface
#endif

    contains

    !> Release the object's state (the reference reallocates scratch here, :136-165).  Called
    !! without `ndim` it also releases the device memory the library keeps between fits of the same
    !! grid (band factor storage, staging buffers); the next fit simply allocates again.
    subroutine destroy_splpak(me,ndim)
        class(splpak_type),intent(inout) :: me
        integer,intent(in),optional :: ndim
        me%mdim = 0
        me%info = 0.0_real64
        me%token = 0
        me%fit_fell_to_host = .false.
        if (present(ndim)) then
            me%mdim = ndim
#ifndef REAL128
        else
            call c_shutdown()
#endif
        end if
    end subroutine destroy_splpak

    !> `call solver%set_host(.true.)`: the following `initialize` / `evaluate_many` / `evaluate_derivatives` calls of this
    !! object run on the HOST solver (splpak_host.F90: banded normal equations + Cholesky + refinement against the rows,
    !! real64 arithmetic) instead of the MI355X -- for machines without a GPU and for small problems.  Explicit only: the
    !! GPU path never falls back to it.  `.false.` returns to the GPU (ignored in a -DREAL128 build, which has no GPU path).
    subroutine splpak_set_host(me,flag)
        class(splpak_type),intent(inout) :: me
        logical,intent(in) :: flag
#ifdef REAL128
        me%host = .true.
#else
        me%host = flag
#endif
    end subroutine splpak_set_host

    !> `call solver%set_option('solver','pcg+direct',ierror)`: a named option of the HIP library (include/splpak_hip.h,
    !! splpak_set_default_option; INTEGRATION.md lists them) for the fits that follow -- process wide, what SPLPAK_<NAME> in the
    !! environment would set.  ierror = 0, or -3 for an unknown name (the library's message is printed).  No effect on the host solver.
    subroutine splpak_set_option(name,value,ierror)
        character(len=*),intent(in) :: name, value
        integer,intent(out) :: ierror
        ierror = 0
#ifndef REAL128
        ierror = int(c_set_default_option(trim(name)//c_null_char, trim(value)//c_null_char))
        if (ierror < 0) call report_library_failure(ierror,'set_option')
#endif
    end subroutine splpak_set_option

    !> The following `initialize` calls of this object use `n` GPUs of the node: the points are sharded
    !! and the band of the normal equations is distributed over them (include/splpak_hip.h,
    !! splpak_fit_multi_f64); n <= 1 is the single-GPU fit.  Same arguments, same results.
    subroutine splpak_set_gpus(me,n)
        class(splpak_type),intent(inout) :: me
        integer,intent(in) :: n
        me%ngpus = max(n,1)
    end subroutine splpak_set_gpus

    !> Diagnostics of the last `initialize` of this object.  `reserr` is the residual norm
    !! ||rows*coef - rhs||_2 over data and constraint rows that the reference computes in suprls
    !! (:1693) and drops in splcw (:690, :1052).
    subroutine splpak_last_fit_info(me,reserr,ndata_rows,nconstraint_rows,refine_steps,optimality,on_host)
        class(splpak_type),intent(in) :: me
        real(wp),intent(out),optional :: reserr        !! residual norm of the fitted system
        integer,intent(out),optional :: ndata_rows       !! data rows used (non-zero weight)
        integer,intent(out),optional :: nconstraint_rows !! derivative-constraint rows of data-sparse nodes (:921-1046)
        integer,intent(out),optional :: refine_steps     !! iterative-refinement steps taken
        real(wp),intent(out),optional :: optimality      !! componentwise backward error of coef w.r.t. the rows
        logical,intent(out),optional :: on_host          !! .true. if this object's fits run on the host solver (set_host)
        if (present(on_host)) on_host = me%host
        if (present(reserr)) reserr = real(me%info(9),wp)
        if (present(ndata_rows)) ndata_rows = int(me%info(1))
        if (present(nconstraint_rows)) nconstraint_rows = int(me%info(2))
        if (present(refine_steps)) refine_steps = int(me%info(3))
        if (present(optimality)) optimality = real(me%info(10),wp)
    end subroutine splpak_last_fit_info

    !> ` IERR=nnnnn` + message on output_unit, as the reference's cfaerr (:399-407).
    subroutine report(ierr,mess)
        integer,intent(in) :: ierr
        character(len=*),intent(in) :: mess
        if (ierr /= 0) write (output_unit,'(A,I5)') ' IERR=', ierr
        write (output_unit,'(A)') trim(mess)
    end subroutine report

    !> a negative status is an infrastructure failure (no GPU, out of device memory, ...)
    !> .true. when a call has to run on the host solver whatever the GPU could do: `set_host(.true.)`, or more than four
    !! dimensions -- the reference takes any ndim >= 1 (:716-722, :1166-1172; "1..4" is a remark in its documentation, :1099),
    !! the HIP kernels are written for 1..4 (include/splpak_hip.h SPLPAK_MAXDIM), the host solver is written for any ndim.
    pure logical function host_takes(me,ndim)
        class(splpak_type),intent(in) :: me
        integer,intent(in) :: ndim
        host_takes = me%host .or. ndim > 4
    end function host_takes

    !> Opt-in for machines without a GPU (fpm dependents running their tests, SURVEY section 8f-4): with
    !! SPLPAK_HOST_IF_NO_GPU=1 in the environment a call that the HIP library refuses with "no usable device" (-1) runs on
    !! the host solver instead, and says so once per process on output_unit.  Never a default, never silent; any other
    !! failure of the library is reported as before.
    logical function host_if_no_gpu(rc)
        integer,intent(in) :: rc
        character(len=8) :: val
        integer :: n, stat
        host_if_no_gpu = .false.
        if (rc /= -1) return
        if (no_gpu_optin < 0) then
            no_gpu_optin = 0
            call get_environment_variable('SPLPAK_HOST_IF_NO_GPU', val, n, stat)
            if (stat == 0 .and. n >= 1) then
                if (val(1:1) == '1') no_gpu_optin = 1
            end if
        end if
        host_if_no_gpu = no_gpu_optin == 1
        if (host_if_no_gpu .and. .not. no_gpu_said) then
            no_gpu_said = .true.
            write(output_unit,'(a)') ' splpak: no usable GPU (HIP library status -1); '// &
                                     'SPLPAK_HOST_IF_NO_GPU=1: running on the host solver'
        end if
    end function host_if_no_gpu

    subroutine report_library_failure(ierr,who)
        integer,intent(in) :: ierr
        character(len=*),intent(in) :: who
        character(kind=c_char) :: buf(512)
        character(len=512) :: msg
        integer :: n, i
        n = 0
        buf = ' '
#ifndef REAL128
        n = c_last_error(buf, 512_c_int32_t)
#endif
        msg = ''
        do i = 1, min(n,511)
            msg(i:i) = buf(i)
        end do
        call report(ierr, ' '//who//' - HIP library failure: '//trim(msg))
    end subroutine report_library_failure

    subroutine report_fit(ierr)
        integer,intent(in) :: ierr
        select case (ierr)
        case (101); call report(ierr,' splcc or splcw - NDIM is less than 1')
        case (102); call report(ierr,' splcc or splcw - NODES(IDIM) is less than 4 for some IDIM')
        case (103); call report(ierr,' splcc or splcw - XMIN(IDIM) equals XMAX(IDIM) for some IDIM')
        case (104); call report(ierr,' splcc or splcw - NCF (size of COEF) is too small')
        case (105); call report(ierr,' splcc or splcw - Ndata Is less than 1')
        case (106); call report(ierr,' splcc or splcw - NWRK (size of WORK) is too small')
        case (107); call report(ierr,' splcc or splcw - suprls failure '//&
                                     '(this usually indicates insufficient input data)')
        end select
    end subroutine report_fit

    !> .true., with ierror = -4 and `mess` reported, where an object cannot take the batch calls (one launch on one GPU):
    !! under set_host or set_gpus(n > 1).  The caller returns at once.
    logical function batch_refused(me,mess,ierror)
        class(splpak_type),intent(in) :: me
        character(len=*),intent(in) :: mess
        integer,intent(inout) :: ierror
        batch_refused = me%host .or. me%ngpus > 1
        if (batch_refused) then
            ierror = -4
            call report(ierror,mess)
        end if
    end function batch_refused

    !> The end of a batch call: ierror = rc, a fit's status reported as `initialize` reports it, a failure of the library
    !! under the procedure's name.
    subroutine report_batch(rc,who,ierror)
        integer(c_int32_t),intent(in) :: rc
        character(len=*),intent(in) :: who
        integer,intent(out) :: ierror
        ierror = int(rc)
        if (rc > 0) then
            call report_fit(ierror)
        else if (rc < 0) then
            call report_library_failure(ierror,who)
        end if
    end subroutine report_batch

    !> Unweighted fit; same arguments as the reference's splcc (:421-422).
    subroutine splcc(me,ndim,xdata,l1xdat,ydata,ndata,xmin,xmax,nodes, &
                     xtrap,coef,ncf,work,nwrk,ierror)
        class(splpak_type),intent(inout) :: me
        integer,intent(in) :: ndim, l1xdat, ncf, nwrk, ndata
        real(wp),intent(in),target :: xdata(l1xdat,*)
        real(wp),intent(in),target :: ydata(*)
        real(wp),intent(in),target :: xmin(*), xmax(*)
        real(wp),intent(in) :: xtrap
        integer,intent(in),target :: nodes(*)
        real(wp),target :: work(*)
        real(wp),intent(out),target :: coef(*)
        integer,intent(out) :: ierror
        call fit_common(me,ndim,c_loc(xdata),l1xdat,c_loc(ydata),c_null_ptr,ndata,c_loc(xmin), &
                        c_loc(xmax),nodes,xtrap,coef,ncf,work,nwrk,ierror)
    end subroutine splcc

    !> Weighted fit; same arguments as the reference's splcw (:512-513).
    !! `wdata(1) < 0` means "no weights" exactly as in the reference (:581-588).
    subroutine splcw(me,ndim,xdata,l1xdat,ydata,wdata,ndata,xmin,xmax, &
                     nodes,xtrap,coef,ncf,work,nwrk,ierror)
        class(splpak_type),intent(inout) :: me
        integer,intent(in) :: ndim, l1xdat, ncf, nwrk, ndata
        real(wp),intent(in),target :: xdata(l1xdat,*)
        real(wp),intent(in),target :: ydata(*)
        real(wp),intent(in) :: wdata(:)
        real(wp),intent(in),target :: xmin(*), xmax(*)
        real(wp),intent(in) :: xtrap
        integer,intent(in),target :: nodes(*)
        real(wp),target :: work(*)
        real(wp),intent(out),target :: coef(*)
        integer,intent(out) :: ierror
        real(wp),allocatable,target :: wcopy(:)
        logical :: weighted
        weighted = .false.
        if (size(wdata) >= 1) weighted = wdata(1) >= 0.0_wp
        if (weighted .and. ndata >= 1) then
            allocate(wcopy(ndata))                 ! contiguous copy of the assumed-shape dummy
            wcopy(1:ndata) = wdata(1:ndata)
            call fit_common(me,ndim,c_loc(xdata),l1xdat,c_loc(ydata),c_loc(wcopy),ndata,c_loc(xmin), &
                            c_loc(xmax),nodes,xtrap,coef,ncf,work,nwrk,ierror)
        else
            call fit_common(me,ndim,c_loc(xdata),l1xdat,c_loc(ydata),c_null_ptr,ndata,c_loc(xmin), &
                            c_loc(xmax),nodes,xtrap,coef,ncf,work,nwrk,ierror)
        end if
    end subroutine splcw

    subroutine fit_common(me,ndim,xdata,l1xdat,ydata,wdata,ndata,xmin,xmax,nodes,xtrap,coef,ncf, &
                          work,nwrk,ierror)
        class(splpak_type),intent(inout),target :: me
        integer,intent(in) :: ndim, l1xdat, ncf, nwrk, ndata
        type(c_ptr),intent(in) :: xdata, ydata, wdata, xmin, xmax
        integer,intent(in),target :: nodes(*)
        real(wp),intent(in) :: xtrap
        real(wp),target :: coef(*), work(*)
        integer,intent(out) :: ierror
        integer(c_int32_t) :: rc
        integer(c_int64_t) :: ncol
        integer :: idim
        type(c_ptr) :: hist
        me%mdim = ndim
        me%token = 0                          ! (whatever this object could refit is being replaced)
        me%fit_fell_to_host = .false.
        ! the histogram comes back in work(1:ncol) when the caller's array can hold it
        hist = c_null_ptr
        ncol = 1
        do idim = 1, max(ndim,0)
            ncol = ncol*int(max(nodes(idim),1),c_int64_t)
        end do
        if (ndim >= 1 .and. xtrap /= 0.0_wp .and. int(nwrk,c_int64_t) >= ncol) hist = c_loc(work)
        if (host_takes(me,ndim)) then
            call fit_on_host(me,ndim,xdata,l1xdat,ydata,wdata,ndata,xmin,xmax,nodes,xtrap,coef,ncf,work,nwrk,ierror)
            return
        end if
#ifndef REAL128
#ifndef REAL32
        if (me%ngpus > 1) then
            rc = c_fit_multi(int(me%ngpus,c_int32_t), int(ndim,c_int32_t), xdata, int(l1xdat,c_int32_t), ydata, wdata, &
                             int(ndata,c_int64_t), xmin, xmax, c_loc(nodes), xtrap, c_loc(coef), &
                             int(ncf,c_int64_t), int(nwrk,c_int64_t), hist, c_loc(me%info))
        else
#endif
        rc = c_fit(int(ndim,c_int32_t), xdata, int(l1xdat,c_int32_t), ydata, wdata, &
                   int(ndata,c_int64_t), xmin, xmax, c_loc(nodes), xtrap, c_loc(coef), &
                   int(ncf,c_int64_t), int(nwrk,c_int64_t), hist, c_loc(me%info))
#ifndef REAL32
        end if
#endif
        ierror = int(rc)
        if (host_if_no_gpu(ierror)) then
            me%fit_fell_to_host = .true.
            call fit_on_host(me,ndim,xdata,l1xdat,ydata,wdata,ndata,xmin,xmax,nodes,xtrap,coef,ncf,work,nwrk,ierror)
            return
        end if
        if (rc == 0 .and. me%ngpus <= 1) then     ! what `refit` continues from
            me%token = c_fit_token()
            me%fit_ndata = int(ndata,c_int64_t)
            me%fit_ncol = ncol
        end if
        if (rc > 0) then
            call report_fit(ierror)
        else if (rc < 0) then
            call report_library_failure(ierror,'splcc or splcw')
        end if
#endif
    end subroutine fit_common

    !> The fit of samples given on a tensor-product grid of points -- an image, a volume, a table: `values` holds one sample
    !! per point of axes_1 x axes_2 x ..., dimension 1 fastest (what `evaluate_grid` writes), `axes` the npts(idim) coordinates
    !! of every dimension back to back (any order, repeats and points outside the box allowed), the optional `waxes` one weight
    !! per axis coordinate in the same layout (the weight of a sample is the product of its coordinates' weights; absent: 1).
    !! Returns what `initialize` returns for the listed product, provided that fit has no constraint rows: xtrap = 0, or
    !! xtrap /= 0 and no data-sparse node (include/splpak_hip.h, splpak_fit_grid_f64; otherwise ierror = -4 with the library's
    !! message: list the points and call `initialize`).  One call of the HIP library: one streaming pass over the samples per
    !! refinement step and ndim small band solves, no sort and no factorisation of the full normal equations.  Under
    !! set_host(.true.), for ndim > 4, in the -DREAL128 build and with SPLPAK_HOST_IF_NO_GPU=1 the product is listed and the
    !! module's host solver fits it (constraint rows included, as `initialize`).  Leaves the object as `initialize` does --
    !! `evaluate*` follow --, except that there is nothing to `refit`.
    !! ierror: 0; 101 .. 105 and 107 as `initialize` (104: ncf smaller than the number of coefficients; 105: an npts(idim) < 1).
    subroutine splpak_fit_grid(me,ndim,npts,axes,values,xmin,xmax,nodes,xtrap,coef,ncf,ierror,waxes)
        class(splpak_type),intent(inout),target :: me
        integer,intent(in) :: ndim, ncf
        integer,intent(in) :: npts(*)
        real(wp),intent(in),target :: axes(*)
        real(wp),intent(in),target :: values(*)
        real(wp),intent(in),target :: xmin(*), xmax(*)
        integer,intent(in),target :: nodes(*)
        real(wp),intent(in) :: xtrap
        real(wp),intent(out),target :: coef(*)
        integer,intent(out) :: ierror
        real(wp),intent(in),optional,target :: waxes(*)
        integer(c_int32_t) :: rc
        integer(c_int64_t),target :: np64(max(ndim,1))
        integer(c_int64_t) :: nsamp, ip
        integer :: idim, ntab, k(max(ndim,1)), off(max(ndim,1))
        logical :: listed
        real(wp),allocatable,target :: xl(:,:), wl(:)
        real(wp),target :: wk(1)
        type(c_ptr) :: pw
        me%mdim = ndim
        me%token = 0                          ! (whatever this object could refit is being replaced)
        me%fit_fell_to_host = .false.
        np64 = 0
        nsamp = 1
        ntab = 0
        do idim = 1, ndim
            np64(idim) = int(npts(idim),c_int64_t)
            off(idim) = ntab
            ntab = ntab + max(npts(idim),0)
            nsamp = nsamp*max(np64(idim),0_c_int64_t)
        end do
        rc = -1
        listed = host_takes(me,ndim)
#ifndef REAL128
        if (.not. listed) then
            pw = c_null_ptr
            if (present(waxes)) pw = c_loc(waxes)
            rc = c_fit_grid(int(ndim,c_int32_t), c_loc(np64), c_loc(axes), pw, 1_c_int32_t, c_loc(values), nsamp, c_loc(xmin), &
                            c_loc(xmax), c_loc(nodes), xtrap, c_loc(coef), int(ncf,c_int64_t), c_loc(me%info))
            if (host_if_no_gpu(int(rc))) then
                listed = .true.
                me%fit_fell_to_host = .true.
            end if
        end if
#endif
        if (listed) then                      ! the host solver on the listed product, first dimension fastest
            ierror = 0
            do idim = 1, ndim
                if (npts(idim) < 1) nsamp = 0
            end do
            allocate(xl(max(ndim,1),max(nsamp,1_c_int64_t)), wl(max(nsamp,1_c_int64_t)))
            k = 1
            do ip = 1, nsamp
                wl(ip) = 1.0_wp
                do idim = 1, ndim
                    xl(idim,ip) = axes(off(idim) + k(idim))
                    if (present(waxes)) wl(ip) = wl(ip)*waxes(off(idim) + k(idim))
                end do
                idim = 1
                do while (idim <= ndim)
                    k(idim) = k(idim) + 1
                    if (k(idim) <= npts(idim)) exit
                    k(idim) = 1
                    idim = idim + 1
                end do
            end do
            ! (a weight list whose first entry is negative would read as "no weights": the grid entry has no such sentinel)
            pw = c_null_ptr
            if (present(waxes) .and. nsamp >= 1) then
                if (wl(1) >= 0.0_wp) then
                    pw = c_loc(wl)
                else
                    ierror = -4
                    call report(ierror,' initialize_grid - a negative weight cannot be listed for the host solver')
                    return
                end if
            end if
            call fit_on_host(me,ndim,c_loc(xl),max(ndim,1),c_loc(values),pw,int(nsamp),c_loc(xmin),c_loc(xmax),nodes,xtrap, &
                             coef,ncf,wk,1,ierror)
            return
        end if
        ierror = int(rc)
        if (rc > 0) then
            call report_fit(ierror)
        else if (rc < 0) then
            call report_library_failure(ierror,'initialize_grid')
        end if
    end subroutine splpak_fit_grid

    !> `initialize_grid` with a weight per sample -- a mask, dead pixels, a variance map: `weights` holds one row weight per
    !! sample in the layout of `values` (the normal equations see its square); a sample whose weight is exactly 0 is left out
    !! and may hold NaN.  Returns what `initialize` returns for the listed samples of non-zero weight, provided that fit has no
    !! constraint rows (include/splpak_hip.h, splpak_fit_grid_weighted_f64: a conjugate-gradient iteration whose operator is
    !! one evaluation and one spread pass over the samples; ierror = -3 for a negative or non-finite weight, -4 where xtrap /= 0
    !! meets data-sparse nodes).  Under set_host(.true.), for ndim > 4, in the -DREAL128 build and with SPLPAK_HOST_IF_NO_GPU=1
    !! the samples of non-zero weight are listed and the module's host solver fits them, as `initialize_grid` does.
    subroutine splpak_fit_grid_weighted(me,ndim,npts,axes,values,weights,xmin,xmax,nodes,xtrap,coef,ncf,ierror)
        class(splpak_type),intent(inout),target :: me
        integer,intent(in) :: ndim, ncf
        integer,intent(in) :: npts(*)
        real(wp),intent(in),target :: axes(*)
        real(wp),intent(in),target :: values(*), weights(*)
        real(wp),intent(in),target :: xmin(*), xmax(*)
        integer,intent(in),target :: nodes(*)
        real(wp),intent(in) :: xtrap
        real(wp),intent(out),target :: coef(*)
        integer,intent(out) :: ierror
        integer(c_int32_t) :: rc
        integer(c_int64_t),target :: np64(max(ndim,1))
        integer(c_int64_t) :: nsamp, ip, nl
        integer :: idim, ntab, k(max(ndim,1)), off(max(ndim,1))
        logical :: listed
        real(wp),allocatable,target :: xl(:,:), wl(:), yl(:)
        real(wp),target :: wk(1)
        me%mdim = ndim
        me%token = 0                          ! (whatever this object could refit is being replaced)
        me%fit_fell_to_host = .false.
        np64 = 0
        nsamp = 1
        ntab = 0
        do idim = 1, ndim
            np64(idim) = int(npts(idim),c_int64_t)
            off(idim) = ntab
            ntab = ntab + max(npts(idim),0)
            nsamp = nsamp*max(np64(idim),0_c_int64_t)
        end do
        rc = -1
        listed = host_takes(me,ndim)
#ifndef REAL128
        if (.not. listed) then
            rc = c_fit_grid_weighted(int(ndim,c_int32_t), c_loc(np64), c_loc(axes), 1_c_int32_t, c_loc(values), nsamp, &
                                     c_loc(weights), 0_c_int64_t, c_loc(xmin), c_loc(xmax), c_loc(nodes), xtrap, c_loc(coef), &
                                     int(ncf,c_int64_t), c_loc(me%info))
            if (host_if_no_gpu(int(rc))) then
                listed = .true.
                me%fit_fell_to_host = .true.
            end if
        end if
#endif
        if (listed) then                      ! the host solver on the listed samples of non-zero weight, first dimension fastest
            ierror = 0
            do idim = 1, ndim
                if (npts(idim) < 1) nsamp = 0
            end do
            allocate(xl(max(ndim,1),max(nsamp,1_c_int64_t)), wl(max(nsamp,1_c_int64_t)), yl(max(nsamp,1_c_int64_t)))
            k = 1
            nl = 0
            do ip = 1, nsamp
                if (weights(ip) < 0.0_wp .or. weights(ip) /= weights(ip) .or. abs(weights(ip)) > huge(1.0_wp)) then
                    ierror = -3
                    call report(ierror,' initialize_grid_weighted - a weight is negative or not finite')
                    return
                end if
                if (weights(ip) /= 0.0_wp) then
                    nl = nl + 1
                    do idim = 1, ndim
                        xl(idim,nl) = axes(off(idim) + k(idim))
                    end do
                    wl(nl) = weights(ip)
                    yl(nl) = values(ip)
                end if
                idim = 1
                do while (idim <= ndim)
                    k(idim) = k(idim) + 1
                    if (k(idim) <= npts(idim)) exit
                    k(idim) = 1
                    idim = idim + 1
                end do
            end do
            call fit_on_host(me,ndim,c_loc(xl),max(ndim,1),c_loc(yl),c_loc(wl),int(nl),c_loc(xmin),c_loc(xmax),nodes,xtrap, &
                             coef,ncf,wk,1,ierror)
            return
        end if
        ierror = int(rc)
        if (rc > 0) then
            call report_fit(ierror)
        else if (rc < 0) then
            call report_library_failure(ierror,'initialize_grid_weighted')
        end if
    end subroutine splpak_fit_grid_weighted

    !> Many small independent fits on one node grid in one launch (include/splpak_hip.h, splpak_fit_many_f64): problem k owns
    !! the points offsets(k)+1 .. offsets(k+1) of xdata(l1xdat,*), ydata and wdata (`offsets(nbatch+1)`, zero based, not
    !! decreasing); its coefficients go to coef(:,k), `ldcoef` apart.  Every problem gets what `initialize` does for its own
    !! points (without `wdata`: splcc); only ndim, nodes, xmin, xmax and xtrap are shared.  ierrors(k): 0, 105 for a problem
    !! without points (its coefficients untouched), 107 with its coefficients zeroed; ierror: 0, or the status of the first
    !! problem that did not end in 0, the argument errors of `initialize`, -3 for a bad offset or leading dimension and -4 for
    !! ndim > 2 or a grid beyond the 64 KiB of LDS a problem may take (the library's message says which) -- never a silent
    !! fallback: loop `initialize` there.  Refused with -4 and a message of its own under set_host, set_gpus(n > 1) and in the
    !! -DREAL128 build, as `refit` is.  The object is left as it was.
    subroutine splpak_fit_many(me,ndim,nbatch,offsets,xdata,l1xdat,ydata,xmin,xmax,nodes,xtrap,coef,ldcoef,ierrors,ierror,wdata)
        class(splpak_type),intent(inout),target :: me
        integer,intent(in) :: ndim, nbatch, l1xdat, ldcoef
        integer(c_int64_t),intent(in),target :: offsets(*)
        real(wp),intent(in),target :: xdata(l1xdat,*), ydata(*)
        real(wp),intent(in),target :: xmin(*), xmax(*)
        integer,intent(in),target :: nodes(*)
        real(wp),intent(in) :: xtrap
        real(wp),intent(inout),target :: coef(ldcoef,*)
        integer,intent(out),target :: ierrors(*)
        integer,intent(out) :: ierror
        real(wp),intent(in),optional,target :: wdata(*)
        integer(c_int32_t) :: rc
        type(c_ptr) :: pw
#ifdef REAL128
        ierror = -4
        call report(ierror,' initialize_many - not available in the -DREAL128 build: call initialize for every problem')
#else
        if (batch_refused(me,' initialize_many - not available under set_host or set_gpus(n > 1): '// &
                             'call initialize for every problem',ierror)) return
        pw = c_null_ptr
        if (present(wdata)) pw = c_loc(wdata)
        rc = c_fit_many(int(ndim,c_int32_t), int(nbatch,c_int32_t), c_loc(offsets), c_loc(xdata), int(l1xdat,c_int32_t), &
                        c_loc(ydata), pw, c_loc(xmin), c_loc(xmax), c_loc(nodes), xtrap, c_loc(coef), int(ldcoef,c_int64_t), &
                        c_loc(ierrors), c_null_ptr)
        call report_batch(rc,'initialize_many',ierror)
#endif
    end subroutine splpak_fit_many

    !> `initialize_many` with sigma clipping, the whole loop in one launch (include/splpak_hip.h, splpak_fit_many_clip_f64,
    !! which states the rule): every problem is fitted, its points whose weighted residual lies more than `khi` (above) or
    !! `klo` (below) times the rms of the counted weighted residuals from the fit are rejected, and it is fitted again, until a
    !! pass rejects nothing or `maxpass` passes have run -- bit for bit the loop initialize_many -> residuals_each -> zero the
    !! rejected weights -> initialize_many.  Arguments as `initialize_many`, and: klo, khi >= 1 (huge(1.0_wp) never rejects; an
    !! infinity switches the side off); maxpass >= 0; wout(*) the weights every problem ended with, indexed like ydata (0 where a
    !! point was rejected; never the array passed as wdata); the optional clip(4,nbatch) = [ residual passes, points rejected,
    !! points counted by the last fit, S / cnt of the last pass ].  ierrors and ierror as `initialize_many`, -3 also for a bad
    !! klo, khi or maxpass; refused with -4 under set_host, set_gpus(n > 1) and in the -DREAL128 build, exactly as it is.
    subroutine splpak_fit_many_clipped(me,ndim,nbatch,offsets,xdata,l1xdat,ydata,xmin,xmax,nodes,xtrap,klo,khi,maxpass,wout, &
                                       coef,ldcoef,ierrors,ierror,wdata,clip)
        class(splpak_type),intent(inout),target :: me
        integer,intent(in) :: ndim, nbatch, l1xdat, ldcoef, maxpass
        integer(c_int64_t),intent(in),target :: offsets(*)
        real(wp),intent(in),target :: xdata(l1xdat,*), ydata(*)
        real(wp),intent(in),target :: xmin(*), xmax(*)
        integer,intent(in),target :: nodes(*)
        real(wp),intent(in) :: xtrap, klo, khi
        real(wp),intent(inout),target :: wout(*)
        real(wp),intent(inout),target :: coef(ldcoef,*)
        integer,intent(out),target :: ierrors(*)
        integer,intent(out) :: ierror
        real(wp),intent(in),optional,target :: wdata(*)
        real(c_double),intent(out),optional,target :: clip(4,*)
        integer(c_int32_t) :: rc
        type(c_ptr) :: pw, pc
#ifdef REAL128
        ierror = -4
        call report(ierror,' initialize_many_clipped - not available in the -DREAL128 build')
#else
        if (batch_refused(me,' initialize_many_clipped - not available under set_host or set_gpus(n > 1)',ierror)) return
        pw = c_null_ptr
        if (present(wdata)) pw = c_loc(wdata)
        pc = c_null_ptr
        if (present(clip)) pc = c_loc(clip)
        rc = c_fit_many_clip(int(ndim,c_int32_t), int(nbatch,c_int32_t), c_loc(offsets), c_loc(xdata), int(l1xdat,c_int32_t), &
                             c_loc(ydata), pw, c_loc(xmin), c_loc(xmax), c_loc(nodes), xtrap, klo, khi, int(maxpass,c_int32_t), &
                             c_loc(wout), c_loc(coef), int(ldcoef,c_int64_t), c_loc(ierrors), c_null_ptr, pc)
        call report_batch(rc,'initialize_many_clipped',ierror)
#endif
    end subroutine splpak_fit_many_clipped

    !> `initialize_many_clipped` on a robust scale (include/splpak_hip.h, splpak_fit_many_clip_mad_f64, which states the rule):
    !! the centre is the median of the weighted residuals, the scale 1.4826 times their MAD, and with regrow /= 0 every point of
    !! non-zero starting weight is judged again in every pass, so a good point rejected beside a run of outliers returns.  The
    !! whole loop runs in one launch, bit for bit the loop initialize_many -> residuals_each -> mad_each -> the rule ->
    !! initialize_many.  Arguments as `initialize_many_clipped` with regrow after maxpass; the optional clip(6,nbatch) =
    !! [ residual passes, points out at the end, points counted by the last fit, s and med of the last pass, points returned in
    !! total ].  ierrors and ierror as `initialize_many_clipped`; refused with -4 under set_host, set_gpus(n > 1) and in the
    !! -DREAL128 build, exactly as it is.
    subroutine splpak_fit_many_robust(me,ndim,nbatch,offsets,xdata,l1xdat,ydata,xmin,xmax,nodes,xtrap,klo,khi,maxpass,regrow,wout, &
                                      coef,ldcoef,ierrors,ierror,wdata,clip)
        class(splpak_type),intent(inout),target :: me
        integer,intent(in) :: ndim, nbatch, l1xdat, ldcoef, maxpass, regrow
        integer(c_int64_t),intent(in),target :: offsets(*)
        real(wp),intent(in),target :: xdata(l1xdat,*), ydata(*)
        real(wp),intent(in),target :: xmin(*), xmax(*)
        integer,intent(in),target :: nodes(*)
        real(wp),intent(in) :: xtrap, klo, khi
        real(wp),intent(inout),target :: wout(*)
        real(wp),intent(inout),target :: coef(ldcoef,*)
        integer,intent(out),target :: ierrors(*)
        integer,intent(out) :: ierror
        real(wp),intent(in),optional,target :: wdata(*)
        real(c_double),intent(out),optional,target :: clip(6,*)
        integer(c_int32_t) :: rc
        type(c_ptr) :: pw, pc
#ifdef REAL128
        ierror = -4
        call report(ierror,' initialize_many_robust - not available in the -DREAL128 build')
#else
        if (batch_refused(me,' initialize_many_robust - not available under set_host or set_gpus(n > 1)',ierror)) return
        pw = c_null_ptr
        if (present(wdata)) pw = c_loc(wdata)
        pc = c_null_ptr
        if (present(clip)) pc = c_loc(clip)
        rc = c_fit_many_clip_mad(int(ndim,c_int32_t), int(nbatch,c_int32_t), c_loc(offsets), c_loc(xdata), int(l1xdat,c_int32_t), &
                                 c_loc(ydata), pw, c_loc(xmin), c_loc(xmax), c_loc(nodes), xtrap, klo, khi, int(maxpass,c_int32_t), &
                                 int(regrow,c_int32_t), c_loc(wout), c_loc(coef), int(ldcoef,c_int64_t), c_loc(ierrors), c_null_ptr, pc)
        call report_batch(rc,'initialize_many_robust',ierror)
#endif
    end subroutine splpak_fit_many_robust

    !> The median and the MAD of every problem's values in one launch (splpak_mad_many_f64): stats(:,k) = [ points counted,
    !! median, MAD, 0 ] of values(offsets(k)+1 : offsets(k+1)) where the optional wsel is not 0 (without it: every point) -- exact
    !! order statistics, all 0 when nothing is counted.  ierror: -3 for a bad offset.  Refused with -4 under set_host,
    !! set_gpus(n > 1) and in the -DREAL128 build, exactly as `residuals_each` is.
    subroutine splpak_mad_each(me,nbatch,offsets,values,stats,ierror,wsel)
        class(splpak_type),intent(inout),target :: me
        integer,intent(in) :: nbatch
        integer(c_int64_t),intent(in),target :: offsets(*)
        real(wp),intent(in),target :: values(*)
        real(c_double),intent(inout),target :: stats(4,*)
        integer,intent(out) :: ierror
        real(wp),intent(in),optional,target :: wsel(*)
        integer(c_int32_t) :: rc
        type(c_ptr) :: pw
#ifdef REAL128
        ierror = -4
        call report(ierror,' mad_each - not available in the -DREAL128 build')
#else
        if (batch_refused(me,' mad_each - not available under set_host or set_gpus(n > 1)',ierror)) return
        pw = c_null_ptr
        if (present(wsel)) pw = c_loc(wsel)
        rc = c_mad_many(int(nbatch,c_int32_t), c_loc(offsets), c_loc(values), pw, c_loc(stats))
        ierror = int(rc)
        if (rc < 0) call report_library_failure(ierror,'mad_each')
#endif
    end subroutine splpak_mad_each

    !> The fits of `initialize_many`, each at its own points, in one launch (include/splpak_hip.h, splpak_eval_many_f64): problem
    !! k owns the points offsets(k)+1 .. offsets(k+1) of x(ldx,*) and f, and has its coefficients in coef(:,k), where
    !! `initialize_many` put them.  f(i) is the very value `evaluate_many` returns for x(:,i) with coef(:,k) (with `nderiv`, that
    !! partial derivative; one pattern for all problems); entries of f outside offsets(1)+1 .. offsets(nbatch+1) are not touched.
    !! (`evaluate_many` is a batch of points of ONE fit, `evaluate_fields` several fits at the SAME points.)  ierror: 101..104 as
    !! splde (104: computed with nderiv clamped), -3 for a bad offset or leading dimension.  Refused with -4 under set_host,
    !! set_gpus(n > 1) and in the -DREAL128 build, exactly as `initialize_many` is.
    subroutine splpak_eval_each(me,ndim,nbatch,offsets,x,ldx,coef,ldcoef,xmin,xmax,nodes,f,ierror,nderiv)
        class(splpak_type),intent(inout),target :: me
        integer,intent(in) :: ndim, nbatch, ldx, ldcoef
        integer(c_int64_t),intent(in),target :: offsets(*)
        real(wp),intent(in),target :: x(ldx,*)
        real(wp),intent(in),target :: coef(ldcoef,*)
        real(wp),intent(in),target :: xmin(*), xmax(*)
        integer,intent(in),target :: nodes(*)
        real(wp),intent(inout),target :: f(*)
        integer,intent(out) :: ierror
        integer,intent(in),optional,target :: nderiv(*)
        integer(c_int32_t) :: rc
        type(c_ptr) :: pd
#ifdef REAL128
        ierror = -4
        call report(ierror,' evaluate_each - not available in the -DREAL128 build: call evaluate_many for every problem')
#else
        if (batch_refused(me,' evaluate_each - not available under set_host or set_gpus(n > 1): '// &
                             'call evaluate_many for every problem',ierror)) return
        pd = c_null_ptr
        if (present(nderiv)) pd = c_loc(nderiv)
        rc = c_eval_many(int(ndim,c_int32_t), int(nbatch,c_int32_t), c_loc(offsets), c_loc(x), int(ldx,c_int32_t), pd, c_loc(coef), &
                         int(ldcoef,c_int64_t), c_loc(xmin), c_loc(xmax), c_loc(nodes), c_loc(f))
        ierror = int(rc)
        select case (ierror)
        case (0)
        case (101); call report(ierror,' splfe or splde - NDIM is less than 1')
        case (102); call report(ierror,' splfe or splde - NODES(IDIM) is less than  4for some IDIM')
        case (103); call report(ierror,' splfe or splde - XMIN(IDIM) = XMAX(IDIM) for some IDIM')
        case (104); call report(ierror,' splde - NDERIV(IDIM) IS less than 0 or greater than 2 for some IDIM')
        case default
            if (ierror < 0) call report_library_failure(ierror,'evaluate_each')
        end select
#endif
    end subroutine splpak_eval_each

    !> `initialize_many` with the covariance of the coefficients (include/splpak_hip.h, splpak_fit_many_cov_f64): beside
    !! coef(:,k), cov(:,k) (`ldcov` apart, ldcov >= ncol (7**ndim + 1) / 2) gets the half stencil of
    !! Z = (A^T W^2 A + C^T C)^-1 of problem k: cov((i-1)*hst + code + 1, k) = Z(i, i + o) for node i (one based, dimension 1
    !! fastest), hst = (7**ndim + 1) / 2 and code = sum_d (o_d + 3) 7**(d-1) <= hst - 1; 0 where i + o is outside the grid.
    !! With wdata = 1 / sigma and no constraint rows Z is the covariance of the coefficients; with constraint rows it never
    !! understates it.  coef, ierrors and ierror are exactly those of `initialize_many`; a problem of status 105 keeps its
    !! cov, one of 107 has it zeroed; ldcov too small is 104.  Refused with -4 where `initialize_many` is.
    subroutine splpak_fit_many_cov(me,ndim,nbatch,offsets,xdata,l1xdat,ydata,xmin,xmax,nodes,xtrap,coef,ldcoef,cov,ldcov, &
                                   ierrors,ierror,wdata)
        class(splpak_type),intent(inout),target :: me
        integer,intent(in) :: ndim, nbatch, l1xdat, ldcoef, ldcov
        integer(c_int64_t),intent(in),target :: offsets(*)
        real(wp),intent(in),target :: xdata(l1xdat,*), ydata(*)
        real(wp),intent(in),target :: xmin(*), xmax(*)
        integer,intent(in),target :: nodes(*)
        real(wp),intent(in) :: xtrap
        real(wp),intent(inout),target :: coef(ldcoef,*)
        real(wp),intent(inout),target :: cov(ldcov,*)
        integer,intent(out),target :: ierrors(*)
        integer,intent(out) :: ierror
        real(wp),intent(in),optional,target :: wdata(*)
        integer(c_int32_t) :: rc
        type(c_ptr) :: pw
#ifdef REAL128
        ierror = -4
        call report(ierror,' initialize_many_cov - not available in the -DREAL128 build')
#else
        if (batch_refused(me,' initialize_many_cov - not available under set_host or set_gpus(n > 1)',ierror)) return
        pw = c_null_ptr
        if (present(wdata)) pw = c_loc(wdata)
        rc = c_fit_many_cov(int(ndim,c_int32_t), int(nbatch,c_int32_t), c_loc(offsets), c_loc(xdata), int(l1xdat,c_int32_t), &
                            c_loc(ydata), pw, c_loc(xmin), c_loc(xmax), c_loc(nodes), xtrap, c_loc(coef), int(ldcoef,c_int64_t), &
                            c_loc(cov), int(ldcov,c_int64_t), c_loc(ierrors), c_null_ptr)
        call report_batch(rc,'initialize_many_cov',ierror)
#endif
    end subroutine splpak_fit_many_cov

    !> The prediction variance of the fits of `initialize_many_cov`, each at its own points, in one launch
    !! (splpak_eval_many_var_f64): v(i) = a^T Z a, a the window row `evaluate_each` forms for x(:,i) with the same `nderiv` (the
    !! variance of that derivative), Z from cov(:,k) of the problem k that owns i.  The variance, not its root, not clamped.
    !! Arguments and ierror as `evaluate_each` with cov, ldcov in the place of coef, ldcoef; ndim is 1 or 2 (-4 otherwise).
    subroutine splpak_variance_each(me,ndim,nbatch,offsets,x,ldx,cov,ldcov,xmin,xmax,nodes,v,ierror,nderiv)
        class(splpak_type),intent(inout),target :: me
        integer,intent(in) :: ndim, nbatch, ldx, ldcov
        integer(c_int64_t),intent(in),target :: offsets(*)
        real(wp),intent(in),target :: x(ldx,*)
        real(wp),intent(in),target :: cov(ldcov,*)
        real(wp),intent(in),target :: xmin(*), xmax(*)
        integer,intent(in),target :: nodes(*)
        real(wp),intent(inout),target :: v(*)
        integer,intent(out) :: ierror
        integer,intent(in),optional,target :: nderiv(*)
        integer(c_int32_t) :: rc
        type(c_ptr) :: pd
#ifdef REAL128
        ierror = -4
        call report(ierror,' variance_each - not available in the -DREAL128 build')
#else
        if (batch_refused(me,' variance_each - not available under set_host or set_gpus(n > 1)',ierror)) return
        pd = c_null_ptr
        if (present(nderiv)) pd = c_loc(nderiv)
        rc = c_eval_many_var(int(ndim,c_int32_t), int(nbatch,c_int32_t), c_loc(offsets), c_loc(x), int(ldx,c_int32_t), pd, &
                             c_loc(cov), int(ldcov,c_int64_t), c_loc(xmin), c_loc(xmax), c_loc(nodes), c_loc(v))
        ierror = int(rc)
        select case (ierror)
        case (0)
        case (101); call report(ierror,' splfe or splde - NDIM is less than 1')
        case (102); call report(ierror,' splfe or splde - NODES(IDIM) is less than  4for some IDIM')
        case (103); call report(ierror,' splfe or splde - XMIN(IDIM) = XMAX(IDIM) for some IDIM')
        case (104); call report(ierror,' splde - NDERIV(IDIM) IS less than 0 or greater than 2 for some IDIM')
        case default
            if (ierror < 0) call report_library_failure(ierror,'variance_each')
        end select
#endif
    end subroutine splpak_variance_each

    !> Residuals and per-problem sums of the fits of `initialize_many` in one launch (splpak_residuals_many_f64): the pass
    !! between two `initialize_many` calls of a clipping loop.  resid(i) = ydata(i) - f(i) for every point, a weight of 0
    !! included; stats(:,k) = [ points counted, S = sum (w r)**2, max |w r|, the smallest ZERO-BASED local index that attains it
    !! (-1 and S = max = 0 when nothing is counted) ].  Weights as `initialize_many`: without `wdata`, or with a negative first
    !! weight of a problem, every point counts with weight 1; a point of weight 0 is left out of the sums.  S is summed in the
    !! order the header fixes (64 strided partial sums, then a butterfly), so stats(:,k) depends on problem k alone.
    !! ierror: 101..103, 104 for ldcoef below the number of coefficients, -3 for a bad offset or leading dimension.  Refused
    !! with -4 under set_host, set_gpus(n > 1) and in the -DREAL128 build, exactly as `initialize_many` is.
    subroutine splpak_residuals_each(me,ndim,nbatch,offsets,xdata,l1xdat,ydata,coef,ldcoef,xmin,xmax,nodes,resid,stats,ierror,wdata)
        class(splpak_type),intent(inout),target :: me
        integer,intent(in) :: ndim, nbatch, l1xdat, ldcoef
        integer(c_int64_t),intent(in),target :: offsets(*)
        real(wp),intent(in),target :: xdata(l1xdat,*), ydata(*)
        real(wp),intent(in),target :: coef(ldcoef,*)
        real(wp),intent(in),target :: xmin(*), xmax(*)
        integer,intent(in),target :: nodes(*)
        real(wp),intent(inout),target :: resid(*)
        real(c_double),intent(inout),target :: stats(4,*)
        integer,intent(out) :: ierror
        real(wp),intent(in),optional,target :: wdata(*)
        integer(c_int32_t) :: rc
        type(c_ptr) :: pw
#ifdef REAL128
        ierror = -4
        call report(ierror,' residuals_each - not available in the -DREAL128 build')
#else
        if (batch_refused(me,' residuals_each - not available under set_host or set_gpus(n > 1)',ierror)) return
        pw = c_null_ptr
        if (present(wdata)) pw = c_loc(wdata)
        rc = c_residuals_many(int(ndim,c_int32_t), int(nbatch,c_int32_t), c_loc(offsets), c_loc(xdata), int(l1xdat,c_int32_t), &
                              c_loc(ydata), pw, c_loc(coef), int(ldcoef,c_int64_t), c_loc(xmin), c_loc(xmax), c_loc(nodes), &
                              c_loc(resid), c_loc(stats))
        call report_batch(rc,'residuals_each',ierror)
#endif
    end subroutine splpak_residuals_each

    !> New values on the points of this object's last `initialize`: several fields sampled at the same points (the
    !! components of a velocity, a time series on a fixed sensor layout, bootstrap replicas) cost one `initialize` and one
    !! `refit` each -- the binning, the normal equations and their factorisation are functions of the points, the weights and
    !! the grid, and the HIP library keeps them on the device (include/splpak_hip.h, splpak_refit_f64).  The reference has no
    !! counterpart.  `ydata(ndata,nfields)`: the values, in the point order of that `initialize`; `coef(ncol,nfields)`: one
    !! set of coefficients per field (`nfields` defaults to 1).  On a grid whose factorisation is the nested dissection the fields of
    !! a call are solved in chunks of up to 8 fields that share every sweep of the factor; every field's coefficients are bit for
    !! bit those of its single-field `refit`, and a chunk with a failing field is run again field by field.  ierror: 0; 107 with the reference's message, as `initialize`;
    !! -3 for nfields < 1; -4, with a message, when there is nothing to refit on the device: no successful `initialize` of
    !! this object, another fit of the process since (the library holds one), `destroy`, or an object under set_host,
    !! set_gpus(n > 1) or with ndim > 4 -- `refit` never falls back to another path silently: call `initialize` per field there.
    subroutine splpak_refit(me,ydata,coef,ierror,nfields)
        class(splpak_type),intent(inout),target :: me
        real(wp),intent(in),target :: ydata(*)
        real(wp),intent(out),target :: coef(*)
        integer,intent(out) :: ierror
        integer,intent(in),optional :: nfields
        integer :: nf, k
        integer(c_int32_t) :: rc
        real(real64),allocatable,target :: info(:,:)
        nf = 1
        if (present(nfields)) nf = nfields
        if (host_takes(me,me%mdim) .or. me%ngpus > 1) then
            ierror = -4
            call report(ierror,' refit - not available under set_host, set_gpus(n > 1) or for ndim > 4: '// &
                               'call initialize for every field')
            return
        end if
        rc = -4
#ifndef REAL128
        if (nf < 1) then
            ierror = -3
            call report(ierror,' refit - NFIELDS is less than 1')
            return
        end if
        if (me%token == 0) then
            ierror = -4
            if (me%fit_fell_to_host) then
                call report(ierror,' refit - the last initialize of this object ran on the host for want of a GPU: '// &
                                   'call initialize for every field')
            else
                call report(ierror,' refit - no successful initialize of this object to refit')
            end if
            return
        end if
        allocate(info(10,nf))
        info = 0.0_real64
        rc = c_refit(me%token, int(nf,c_int32_t), c_loc(ydata), me%fit_ndata, me%fit_ndata, c_loc(coef), me%fit_ncol, c_loc(info))
        ! last_fit_info: of the last field that was solved -- the last one, or the one that ended in 107 (the fields behind
        ! it are not run and their diagnostics are zero, row counts included)
        if (rc == 0 .or. rc == 107) then
            do k = nf, 1, -1
                if (info(1,k) > 0.0_real64 .or. k == 1) then
                    me%info = info(:,k)
                    exit
                end if
            end do
        end if
#endif
        ierror = int(rc)
        if (rc > 0) then
            call report_fit(ierror)
        else if (rc < 0) then
            call report_library_failure(ierror,'refit')
        end if
    end subroutine splpak_refit

    !> The fit on the host solver (set_host / REAL128): the reference's argument checks in its order (:716-781), then
    !! splpak_host_solver's banded normal equations.  Same `ierror` codes and messages as the GPU path.
    subroutine fit_on_host(me,ndim,xdata,l1xdat,ydata,wdata,ndata,xmin,xmax,nodes,xtrap,coef,ncf,work,nwrk,ierror)
        class(splpak_type),intent(inout) :: me
        integer,intent(in) :: ndim, l1xdat, ncf, nwrk, ndata
        type(c_ptr),intent(in) :: xdata, ydata, wdata, xmin, xmax
        integer,intent(in) :: nodes(*)
        real(wp),intent(in) :: xtrap
        real(wp) :: coef(*), work(*)
        integer,intent(out) :: ierror
        real(wp),pointer :: px(:,:), py(:), pw(:), pmin(:), pmax(:)
        real(wp),target :: wdummy(1)
        real(wp),allocatable :: hst(:)
        integer :: idim, nwrk1
        integer(c_int64_t) :: ncol
        logical :: weighted, want
        ierror = 0
        if (ndim < 1) ierror = 101
        if (ierror == 0) then
            call c_f_pointer(xmin, pmin, [ndim])
            call c_f_pointer(xmax, pmax, [ndim])
            ncol = 1
            do idim = 1, ndim
                if (nodes(idim) < 4) then
                    ierror = 102
                    exit
                end if
                if (pmax(idim) - pmin(idim) == 0.0_wp) then
                    ierror = 103
                    exit
                end if
                ncol = ncol*int(nodes(idim),c_int64_t)
            end do
        end if
        if (ierror == 0) then
            if (ncol > int(ncf,c_int64_t)) ierror = 104
        end if
        if (ierror == 0 .and. ndata < 1) ierror = 105
        if (ierror == 0) then
            nwrk1 = 1
            if (xtrap /= 0.0_wp) nwrk1 = int(min(ncol+1, int(huge(1),c_int64_t)))
            if (nwrk - nwrk1 + 1 < 1) ierror = 106
        end if
        if (ierror /= 0) then
            call report_fit(ierror)
            return
        end if
        call c_f_pointer(xdata, px, [l1xdat, ndata])
        call c_f_pointer(ydata, py, [ndata])
        weighted = c_associated(wdata)
        if (weighted) then
            call c_f_pointer(wdata, pw, [ndata])
        else
            wdummy = -1.0_wp
            pw => wdummy
        end if
        want = xtrap /= 0.0_wp .and. int(nwrk,c_int64_t) >= ncol
        allocate(hst(int(ncol)))
        call host_fit(ndim, px, l1xdat, py, pw, weighted, ndata, pmin, pmax, nodes, xtrap, coef, hst, want, me%info, ierror)
        if (want) work(1:int(ncol)) = hst
        if (ierror /= 0) call report_fit(ierror)
    end subroutine fit_on_host

    !> Spline value at one point; same arguments as the reference's splfe (:1258).  Host computation.
    function splfe(me,ndim,x,coef,xmin,xmax,nodes,ierror)
        class(splpak_type),intent(inout) :: me
        real(wp) :: splfe
        integer,intent(in) :: ndim
        real(wp),intent(in) :: x(*)
        real(wp),intent(out) :: coef(*)            ! intent as in the reference (:1264); only read
        real(wp),intent(in) :: xmin(*), xmax(*)
        integer,intent(in) :: nodes(*)
        integer,intent(out) :: ierror
        integer :: nderiv(max(ndim,1))
        nderiv = 0
        splfe = eval_point(me,ndim,x,nderiv,coef,xmin,xmax,nodes,ierror)
    end function splfe

    !> Partial derivative at one point; same arguments as the reference's splde (:1089).  Host computation.
    function splde(me,ndim,x,nderiv,coef,xmin,xmax,nodes,ierror)
        class(splpak_type),intent(inout) :: me
        real(wp) :: splde
        integer,intent(in) :: ndim
        real(wp),intent(in) :: x(*)
        integer,intent(in) :: nderiv(*)
        real(wp),intent(out) :: coef(*)
        real(wp),intent(in) :: xmin(*), xmax(*)
        integer,intent(in) :: nodes(*)
        integer,intent(out) :: ierror
        splde = eval_point(me,ndim,x,nderiv,coef,xmin,xmax,nodes,ierror)
    end function splde

    !> The scalar evaluation: checks and `ierror` as splde (:1166-1194: 101/102/103 return 0, 104 is
    !! reported and the value is still computed), then the separable form of the reference's window
    !! sum (:1197-1236): per dimension the (at most) four 1-D factors of the window
    !! [ibmn, ibmx] (:1201-1209) are tabulated once, and the 4^ndim products are accumulated with the
    !! first dimension running fastest.  Any ndim >= 1 (the reference documents 1..4, :1099).
    function eval_point(me,ndim,x,nderiv,coef,xmin,xmax,nodes,ierror) result(f)
        class(splpak_type),intent(inout) :: me
        integer,intent(in) :: ndim
        real(wp),intent(in) :: x(*)
        integer,intent(in) :: nderiv(*)
        real(wp),intent(in) :: coef(*)
        real(wp),intent(in) :: xmin(*), xmax(*)
        integer,intent(in) :: nodes(*)
        integer,intent(out) :: ierror
        real(wp) :: f
        real(hk) :: tab(4,max(ndim,1)), dx, s, t, prod, acc
        integer :: first(max(ndim,1)), width(max(ndim,1)), k(max(ndim,1)), stride(max(ndim,1))
        integer :: idim, it, ibmn, ibmx, j, icol, ider
        f = 0.0_wp
        ierror = 0
        me%mdim = ndim
        if (ndim < 1) then
            ierror = 101
            call report(ierror,' splfe or splde - NDIM is less than 1')
            return
        end if
        do idim = 1, ndim
            if (nodes(idim) < 4) then
                ierror = 102
                call report(ierror,' splfe or splde - NODES(IDIM) is less than  4for some IDIM')
                return
            end if
            if (xmax(idim) - xmin(idim) == 0.0_wp) then
                ierror = 103
                call report(ierror,' splfe or splde - XMIN(IDIM) = XMAX(IDIM) for some IDIM')
                return
            end if
        end do
        do idim = 1, ndim
            if (nderiv(idim) < 0 .or. nderiv(idim) > 2) then
                ierror = 104
                call report(ierror,' splde - NDERIV(IDIM) IS less than 0 or greater than 2 for some IDIM')
                exit                                        ! the reference reports and computes on (:1190-1194)
            end if
        end do
        icol = 1
        do idim = 1, ndim
            stride(idim) = icol
            icol = icol*nodes(idim)
            dx = (real(xmax(idim),hk) - real(xmin(idim),hk))/real(nodes(idim)-1,hk)
            s = 1.0_hk/dx
            t = s*(real(x(idim),hk) - real(xmin(idim),hk))
            it = int(max(min(t,2.0e9_hk),-2.0e9_hk))     ! truncation toward zero, saturating
            ibmn = min(max(it-1,0),nodes(idim)-2)
            ibmx = max(min(it+2,nodes(idim)-1),1)
            first(idim) = ibmn
            width(idim) = ibmx - ibmn + 1
            ider = min(max(nderiv(idim),0),2)
            do j = 1, width(idim)
                tab(j,idim) = host_basis(ibmn+j-1, nodes(idim), ider, real(x(idim),hk), &
                                         real(xmin(idim),hk) + real(ibmn+j-1,hk)*dx, s)
            end do
        end do
        acc = 0.0_hk
        k = 1
        do
            prod = 1.0_hk
            icol = 1
            do idim = 1, ndim
                prod = prod*tab(k(idim),idim)
                icol = icol + (first(idim) + k(idim) - 1)*stride(idim)
            end do
            acc = acc + real(coef(icol),hk)*prod
            idim = 1                                        ! odometer, first dimension fastest (:1228-1232)
            do while (idim <= ndim)
                k(idim) = k(idim) + 1
                if (k(idim) <= width(idim)) exit
                k(idim) = 1
                idim = idim + 1
            end do
            if (idim > ndim) exit
        end do
        f = real(acc,wp)
    end function eval_point

    !> Batch of values: x(ldx,nq) -> f(nq).  One kernel launch for all points.
    subroutine splfe_many(me,ndim,nq,x,ldx,coef,xmin,xmax,nodes,f,ierror)
        class(splpak_type),intent(inout) :: me
        integer,intent(in) :: ndim, nq, ldx
        real(wp),intent(in),target :: x(ldx,*)
        real(wp),intent(in),target :: coef(*)
        real(wp),intent(in),target :: xmin(*), xmax(*)
        integer,intent(in),target :: nodes(*)
        real(wp),intent(out),target :: f(*)
        integer,intent(out) :: ierror
        call eval_common(me,ndim,int(nq,c_int64_t),c_loc(x),ldx,c_null_ptr,c_loc(coef),c_loc(xmin), &
                         c_loc(xmax),c_loc(nodes),c_loc(f),ierror)
    end subroutine splfe_many

    !> Batch of partial derivatives (one `nderiv` pattern for all points).
    subroutine splde_many(me,ndim,nq,x,ldx,nderiv,coef,xmin,xmax,nodes,f,ierror)
        class(splpak_type),intent(inout) :: me
        integer,intent(in) :: ndim, nq, ldx
        real(wp),intent(in),target :: x(ldx,*)
        integer,intent(in),target :: nderiv(*)
        real(wp),intent(in),target :: coef(*)
        real(wp),intent(in),target :: xmin(*), xmax(*)
        integer,intent(in),target :: nodes(*)
        real(wp),intent(out),target :: f(*)
        integer,intent(out) :: ierror
        call eval_common(me,ndim,int(nq,c_int64_t),c_loc(x),ldx,c_loc(nderiv),c_loc(coef),c_loc(xmin), &
                         c_loc(xmax),c_loc(nodes),c_loc(f),ierror)
    end subroutine splde_many

    !> Value, gradient and (order = 2) Hessian of a batch of points in one pass: column i of
    !! f(ldf,nq) holds [ f, df/dx_1..df/dx_ndim, then for order 2 the upper triangle of the Hessian
    !! row by row ] at x(:,i) -- what 1 + ndim (+ ndim(ndim+1)/2) `evaluate` calls with the
    !! matching nderiv would return (splde, reference :1089-1240).
    subroutine splpak_derivs_many(me,ndim,nq,x,ldx,order,coef,xmin,xmax,nodes,f,ldf,ierror)
        class(splpak_type),intent(inout) :: me
        integer,intent(in) :: ndim, nq, ldx, order, ldf
        real(wp),intent(in),target :: x(ldx,*)
        real(wp),intent(in),target :: coef(*)
        real(wp),intent(in),target :: xmin(*), xmax(*)
        integer,intent(in),target :: nodes(*)
        real(wp),intent(out),target :: f(ldf,*)
        integer,intent(out) :: ierror
        integer(c_int32_t) :: rc
        integer :: iq, idm, jdm, col, nder(max(ndim,1)), ie
        me%mdim = ndim
        rc = 0
#ifndef REAL128
        if (.not. host_takes(me,ndim)) then
            rc = c_eval_derivs(int(ndim,c_int32_t), int(nq,c_int64_t), c_loc(x), int(ldx,c_int32_t), &
                               int(order,c_int32_t), c_loc(coef), c_loc(xmin), c_loc(xmax), c_loc(nodes), &
                               c_loc(f), int(ldf,c_int32_t))
        end if
#endif
        if (host_takes(me,ndim) .or. host_if_no_gpu(int(rc))) then      ! host solver: every column is the scalar splde of its pattern
            ierror = 0
            if (order < 1 .or. order > 2 .or. ldf < 1 + ndim + merge(ndim*(ndim+1)/2, 0, order == 2)) then
                ierror = -3
                call report(ierror,' evaluate_derivatives - order must be 1 or 2 and ldf large enough')
                return
            end if
            do iq = 1, nq
                nder = 0
                f(1,iq) = eval_point(me,ndim,x(:,iq),nder,coef,xmin,xmax,nodes,ie)
                if (ie /= 0) then
                    ierror = ie
                    return
                end if
                do idm = 1, ndim
                    nder = 0
                    nder(idm) = 1
                    f(1+idm,iq) = eval_point(me,ndim,x(:,iq),nder,coef,xmin,xmax,nodes,ie)
                end do
                if (order == 2) then
                    col = 1 + ndim
                    do idm = 1, ndim
                        do jdm = idm, ndim
                            nder = 0
                            nder(idm) = nder(idm) + 1
                            nder(jdm) = nder(jdm) + 1
                            col = col + 1
                            f(col,iq) = eval_point(me,ndim,x(:,iq),nder,coef,xmin,xmax,nodes,ie)
                        end do
                    end do
                end if
            end do
            return
        end if
#ifdef REAL128
        rc = -1
#endif
        ierror = int(rc)
        select case (ierror)
        case (0)
        case (101); call report(ierror,' splfe or splde - NDIM is less than 1')
        case (102); call report(ierror,' splfe or splde - NODES(IDIM) is less than  4for some IDIM')
        case (103); call report(ierror,' splfe or splde - XMIN(IDIM) = XMAX(IDIM) for some IDIM')
        case default
            if (ierror < 0) call report_library_failure(ierror,'evaluate_derivatives')
        end select
    end subroutine splpak_derivs_many

    !> Resampling a fit onto a grid: f(i1 + npts(1)*((i2-1) + npts(2)*((i3-1) + ...))) is the spline -- with `nderiv`, that
    !! partial derivative -- at (axes_1(i1), axes_2(i2), ...), what a loop of `evaluate` calls over a regular sample
    !! returns (splfe :1258, splde :1089).  `axes` holds the npts(1) coordinates of dimension 1, then the npts(2) of
    !! dimension 2, ... (any order, repeats and points outside the grid allowed); `f` has product(npts) entries, dimension 1
    !! fastest, the ordering of `coef`.  One call of the HIP library (splpak_eval_grid_f64: no point list is formed);
    !! under set_host(.true.), for ndim > 4 or with SPLPAK_HOST_IF_NO_GPU=1 a loop over the module's scalar evaluation,
    !! as in evaluate_many.  ierror: 101..104 as splde (104: computed with nderiv clamped), -3 for a negative npts.
    subroutine splpak_eval_grid(me,ndim,npts,axes,coef,xmin,xmax,nodes,f,ierror,nderiv)
        class(splpak_type),intent(inout) :: me
        integer,intent(in) :: ndim
        integer,intent(in) :: npts(*)
        real(wp),intent(in),target :: axes(*)
        real(wp),intent(in),target :: coef(*)
        real(wp),intent(in),target :: xmin(*), xmax(*)
        integer,intent(in),target :: nodes(*)
        real(wp),intent(out),target :: f(*)
        integer,intent(out) :: ierror
        integer,intent(in),optional,target :: nderiv(*)
        integer(c_int32_t) :: rc
        integer(c_int64_t),target :: np64(max(ndim,1))
        integer(c_int64_t) :: iq, nq
        integer :: idim, ie, nder(max(ndim,1)), k(max(ndim,1)), off(max(ndim,1))
        real(wp) :: x(max(ndim,1))
        type(c_ptr) :: pd
        me%mdim = ndim
        rc = 0
        np64 = 0
        do idim = 1, ndim
            np64(idim) = int(npts(idim),c_int64_t)
        end do
        pd = c_null_ptr
        if (present(nderiv)) pd = c_loc(nderiv)
#ifndef REAL128
        if (.not. (host_takes(me,ndim) .and. ndim >= 1)) &
            rc = c_eval_grid(int(ndim,c_int32_t), c_loc(np64), c_loc(axes), pd, c_loc(coef), c_loc(xmin), c_loc(xmax), &
                             c_loc(nodes), c_loc(f))
#endif
        if ((host_takes(me,ndim) .or. host_if_no_gpu(int(rc))) .and. ndim >= 1) then   ! host solver: a loop over the scalar evaluation
            ierror = 0
            nq = 1
            do idim = 1, ndim
                if (npts(idim) < 0) then
                    ierror = -3
                    call report(ierror,' evaluate_grid - NPTS(IDIM) is negative for some IDIM')
                    return
                end if
                off(idim) = int(sum(np64(1:idim-1)))
                nq = nq*np64(idim)
            end do
            nder = 0
            if (present(nderiv)) nder = nderiv(1:ndim)
            k = 1
            do iq = 1, nq
                do idim = 1, ndim
                    x(idim) = axes(off(idim) + k(idim))
                end do
                f(iq) = eval_point(me,ndim,x,nder,coef,xmin,xmax,nodes,ie)
                if (ie /= 0) ierror = ie
                if (ie /= 0 .and. ie /= 104) return
                idim = 1                                    ! odometer, first dimension fastest
                do while (idim <= ndim)
                    k(idim) = k(idim) + 1
                    if (k(idim) <= npts(idim)) exit
                    k(idim) = 1
                    idim = idim + 1
                end do
            end do
            return
        end if
#ifdef REAL128
        rc = -1
#endif
        ierror = int(rc)
        select case (ierror)
        case (0)
        case (101); call report(ierror,' splfe or splde - NDIM is less than 1')
        case (102); call report(ierror,' splfe or splde - NODES(IDIM) is less than  4for some IDIM')
        case (103); call report(ierror,' splfe or splde - XMIN(IDIM) = XMAX(IDIM) for some IDIM')
        case (104); call report(ierror,' splde - NDERIV(IDIM) IS less than 0 or greater than 2 for some IDIM')
        case default
            if (ierror < 0) call report_library_failure(ierror,'evaluate_grid')
        end select
    end subroutine splpak_eval_grid

    !> Value, gradient and (order = 2) Hessian of a fit on the grid of `evaluate_grid`, in planes: f(i,e) is entry e of
    !! `evaluate_derivatives` -- the value, d/dx_1 .. d/dx_ndim, then for order 2 the upper triangle of the Hessian row by
    !! row -- at grid point i = i1 + npts(1)*((i2-1) + npts(2)*((i3-1) + ...)), what `evaluate_grid` returns there under the
    !! matching `nderiv`.  f is f(ldf,nplanes) with ldf >= product(npts); rows of f beyond product(npts) are not touched.
    !! One call of the HIP library (splpak_eval_grid_derivs_f64); under set_host(.true.), in the -DREAL128 build, for
    !! ndim > 4 or with SPLPAK_HOST_IF_NO_GPU=1 the loop of `evaluate_grid` on the host, once per pattern.
    !! ierror: 101..103 as splde, -3 for a negative npts, an order outside 1..2 or an ldf too small.
    subroutine splpak_eval_grid_derivs(me,ndim,npts,axes,order,coef,xmin,xmax,nodes,f,ldf,ierror)
        class(splpak_type),intent(inout) :: me
        integer,intent(in) :: ndim, order, ldf
        integer,intent(in) :: npts(*)
        real(wp),intent(in),target :: axes(*)
        real(wp),intent(in),target :: coef(*)
        real(wp),intent(in),target :: xmin(*), xmax(*)
        integer,intent(in),target :: nodes(*)
        real(wp),intent(inout),target :: f(ldf,*)
        integer,intent(out) :: ierror
        integer(c_int32_t) :: rc
        integer(c_int64_t),target :: np64(max(ndim,1))
        integer(c_int64_t) :: iq, nq
        integer :: idim, jdm, ie, col, nplanes, nder(max(ndim,1)), k(max(ndim,1)), off(max(ndim,1))
        real(wp) :: x(max(ndim,1))
        me%mdim = ndim
        rc = 0
        np64 = 0
        do idim = 1, ndim
            np64(idim) = int(npts(idim),c_int64_t)
        end do
#ifndef REAL128
        if (.not. (host_takes(me,ndim) .and. ndim >= 1)) &
            rc = c_eval_grid_derivs(int(ndim,c_int32_t), c_loc(np64), c_loc(axes), int(order,c_int32_t), c_loc(coef), &
                                    c_loc(xmin), c_loc(xmax), c_loc(nodes), c_loc(f), int(ldf,c_int64_t))
#endif
        if ((host_takes(me,ndim) .or. host_if_no_gpu(int(rc))) .and. ndim >= 1) then   ! host solver: the scalar evaluation per pattern
            ierror = 0
            nq = 1
            do idim = 1, ndim
                if (npts(idim) < 0) then
                    ierror = -3
                    call report(ierror,' evaluate_grid_derivatives - NPTS(IDIM) is negative for some IDIM')
                    return
                end if
                off(idim) = int(sum(np64(1:idim-1)))
                nq = nq*np64(idim)
            end do
            if (order < 1 .or. order > 2 .or. int(ldf,c_int64_t) < nq) then
                ierror = -3
                call report(ierror,' evaluate_grid_derivatives - order must be 1 or 2 and ldf at least product(NPTS)')
                return
            end if
            nplanes = 1 + ndim + merge(ndim*(ndim+1)/2, 0, order == 2)
            idim = 0                                        ! the pattern of plane `col`, as evaluate_derivatives forms them
            jdm = 0
            do col = 1, nplanes
                nder = 0
                if (col > 1 .and. col <= 1 + ndim) then
                    nder(col-1) = 1
                else if (col > 1 + ndim) then
                    if (col == 2 + ndim) then
                        idim = 1
                        jdm = 1
                    else if (jdm == ndim) then
                        idim = idim + 1
                        jdm = idim
                    else
                        jdm = jdm + 1
                    end if
                    nder(idim) = nder(idim) + 1
                    nder(jdm) = nder(jdm) + 1
                end if
                k = 1
                do iq = 1, nq
                    do ie = 1, ndim
                        x(ie) = axes(off(ie) + k(ie))
                    end do
                    f(iq,col) = eval_point(me,ndim,x,nder,coef,xmin,xmax,nodes,ie)
                    if (ie /= 0) then
                        ierror = ie
                        return
                    end if
                    ie = 1                                  ! odometer, first dimension fastest
                    do while (ie <= ndim)
                        k(ie) = k(ie) + 1
                        if (k(ie) <= npts(ie)) exit
                        k(ie) = 1
                        ie = ie + 1
                    end do
                end do
            end do
            return
        end if
#ifdef REAL128
        rc = -1
#endif
        ierror = int(rc)
        select case (ierror)
        case (0)
        case (101); call report(ierror,' splfe or splde - NDIM is less than 1')
        case (102); call report(ierror,' splfe or splde - NODES(IDIM) is less than  4for some IDIM')
        case (103); call report(ierror,' splfe or splde - XMIN(IDIM) = XMAX(IDIM) for some IDIM')
        case default
            if (ierror < 0) call report_library_failure(ierror,'evaluate_grid_derivatives')
        end select
    end subroutine splpak_eval_grid_derivs

    !> Integrals of a fit over the cells of a tensor grid: dimension idim with mode(idim) = 1 is INTEGRATED -- its axis holds
    !! ncell(idim)+1 edges and output index j is the cell from e(j) to e(j+1) -- and one with mode(idim) = 0 is EVALUATED at
    !! its ncell(idim) coordinates, as in `evaluate_grid`.  `axes` holds the axes back to back; `f` has product(ncell)
    !! entries, dimension 1 fastest.  Edges may be unsorted, repeated (an empty cell is 0), reversed (the negation) and
    !! outside the grid (the integral of the linear extrapolation).  Exact: every cell is cut at the node lines and each
    !! piece integrated by two-point Gauss-Legendre.  A mean is the caller's division by the cell volume.
    !! One call of the HIP library (splpak_integrate_grid_f64); under set_host(.true.), in the -DREAL128 build, for ndim > 4
    !! or with SPLPAK_HOST_IF_NO_GPU=1 the same pieces and the same rule over the module's scalar evaluation.
    !! ierror: 101..103 as splfe, -3 for a negative ncell or a mode outside 0 and 1.
    subroutine splpak_integrate_grid(me,ndim,ncell,mode,axes,coef,xmin,xmax,nodes,f,ierror)
        class(splpak_type),intent(inout) :: me
        integer,intent(in) :: ndim
        integer,intent(in) :: ncell(*), mode(*)
        real(wp),intent(in),target :: axes(*)
        real(wp),intent(in),target :: coef(*)
        real(wp),intent(in),target :: xmin(*), xmax(*)
        integer,intent(in),target :: nodes(*)
        real(wp),intent(out),target :: f(*)
        integer,intent(out) :: ierror
        integer(c_int32_t) :: rc
        integer(c_int64_t),target :: nc64(max(ndim,1))
        integer(c_int32_t),target :: md32(max(ndim,1))
        integer(c_int64_t) :: iq, nq
        integer :: idim, ie, mxq, nder(max(ndim,1)), k(max(ndim,1)), kq(max(ndim,1)), nqd(max(ndim,1)), off(max(ndim,1))
        real(wp) :: x(max(ndim,1)), acc(max(ndim,1)), v
        real(wp),allocatable :: xq(:,:), wq(:,:)
        me%mdim = ndim
        rc = 0
        nc64 = 0
        md32 = 1
        do idim = 1, ndim
            nc64(idim) = int(ncell(idim),c_int64_t)
            md32(idim) = int(mode(idim),c_int32_t)
        end do
#ifndef REAL128
        if (.not. (host_takes(me,ndim) .and. ndim >= 1)) &
            rc = c_integrate_grid(int(ndim,c_int32_t), c_loc(nc64), c_loc(md32), c_loc(axes), c_loc(coef), c_loc(xmin), &
                                  c_loc(xmax), c_loc(nodes), c_loc(f))
#endif
        if ((host_takes(me,ndim) .or. host_if_no_gpu(int(rc))) .and. ndim >= 1) then   ! host solver: the rule over the scalar evaluation
            ierror = 0
            nq = 1
            ie = 0
            do idim = 1, ndim
                if (ncell(idim) < 0 .or. mode(idim) < 0 .or. mode(idim) > 1) then
                    ierror = -3
                    call report(ierror,' integrate_grid - NCELL(IDIM) is negative or MODE(IDIM) is not 0 or 1 for some IDIM')
                    return
                end if
                off(idim) = ie
                ie = ie + ncell(idim) + mode(idim)
                nq = nq*nc64(idim)
            end do
            nder = 0
            x(1:ndim) = xmin(1:ndim)
            v = eval_point(me,ndim,x,nder,coef,xmin,xmax,nodes,ie)     ! the checks of the grid (102, 103)
            if (ie /= 0) then
                ierror = ie
                f(1:nq) = 0.0_wp
                return
            end if
            mxq = 2*(maxval(nodes(1:ndim)) + 1)                        ! at most nodes + 1 pieces per cell
            allocate(xq(mxq,ndim), wq(mxq,ndim))
            k = 1
            do iq = 1, nq
                do idim = 1, ndim
                    if (mode(idim) == 0) then
                        nqd(idim) = 1
                        xq(1,idim) = axes(off(idim) + k(idim))
                        wq(1,idim) = 1.0_wp
                    else
                        call cell_rule(axes(off(idim) + k(idim)), axes(off(idim) + k(idim) + 1), xmin(idim), xmax(idim), &
                                       nodes(idim), nqd(idim), xq(:,idim), wq(:,idim))
                    end if
                end do
                ! the tensor of the points: dimension 1 innermost, one accumulator per dimension
                acc = 0.0_wp
                kq = 1
                tensor: do
                    do idim = 1, ndim
                        x(idim) = xq(kq(idim),idim)
                    end do
                    v = eval_point(me,ndim,x,nder,coef,xmin,xmax,nodes,ie)
                    acc(1) = acc(1) + wq(kq(1),1)*v
                    idim = 1
                    do
                        kq(idim) = kq(idim) + 1
                        if (kq(idim) <= nqd(idim)) exit
                        kq(idim) = 1
                        if (idim == ndim) exit tensor
                        acc(idim+1) = acc(idim+1) + wq(kq(idim+1),idim+1)*acc(idim)
                        acc(idim) = 0.0_wp
                        idim = idim + 1
                    end do
                end do tensor
                f(iq) = acc(ndim)
                idim = 1                                    ! odometer over the cells, first dimension fastest
                do while (idim <= ndim)
                    k(idim) = k(idim) + 1
                    if (k(idim) <= ncell(idim)) exit
                    k(idim) = 1
                    idim = idim + 1
                end do
            end do
            return
        end if
#ifdef REAL128
        rc = -1
#endif
        ierror = int(rc)
        select case (ierror)
        case (0)
        case (101); call report(ierror,' splfe or splde - NDIM is less than 1')
        case (102); call report(ierror,' splfe or splde - NODES(IDIM) is less than  4for some IDIM')
        case (103); call report(ierror,' splfe or splde - XMIN(IDIM) = XMAX(IDIM) for some IDIM')
        case default
            if (ierror < 0) call report_library_failure(ierror,'integrate_grid')
        end select
    end subroutine splpak_integrate_grid

    !> The two Gauss-Legendre points and weights of every piece of the cell e0 .. e1 of one dimension: the cell is cut at the
    !! node lines xmin + k*dx, the region of a coordinate is k = floor((x - xmin)/dx) clamped to -1 .. nodes-1, the weights
    !! carry the sign of e1 - e0.  The construction of csrc/pieces.hpp, not its arithmetic: the device forms the region
    !! from dxin*(x - xmin), so for an edge within a rounding of a node line the two may cut one piece more or less -- a
    !! piece of a few ulps, which changes the integral by less than a rounding.  Everything here is in the working
    !! precision wp: under -DREAL32 the host form accumulates in single precision, unlike the device.
    subroutine cell_rule(e0,e1,xmin,xmax,nodes,n,xq,wq)
        real(wp),intent(in) :: e0, e1, xmin, xmax
        integer,intent(in) :: nodes
        integer,intent(out) :: n
        real(wp),intent(out) :: xq(:), wq(:)
        real(wp) :: lo, hi, dx, a, b, m, h, sgn
        integer :: klo, khi, q, r
        lo = min(e0,e1)
        hi = max(e0,e1)
        sgn = merge(1.0_wp, -1.0_wp, e0 <= e1)
        dx = (xmax - xmin)/real(nodes - 1,wp)
        klo = region(lo)
        khi = max(region(hi), klo)
        n = 0
        do q = 0, khi - klo
            r = klo + q
            a = lo
            b = hi
            if (q > 0) a = min(max(xmin + real(r,wp)*dx, lo), hi)
            if (q < khi - klo) b = min(max(xmin + real(r+1,wp)*dx, lo), hi)
            m = 0.5_wp*(a + b)
            h = 0.5_wp*(b - a)
            xq(n+1) = m - h/sqrt(3.0_wp)
            xq(n+2) = m + h/sqrt(3.0_wp)
            wq(n+1) = sgn*h
            wq(n+2) = sgn*h
            n = n + 2
        end do
    contains
        integer function region(x)
            real(wp),intent(in) :: x
            real(wp) :: t
            t = (x - xmin)/dx
            if (.not. (t >= 0.0_wp)) then
                region = -1
            else if (t >= real(nodes - 1,wp)) then
                region = nodes - 1
            else
                region = int(t)
            end if
        end function region
    end subroutine cell_rule

    !> The integral of a fit over the box lower(idim) .. upper(idim): `integrate_grid` with one cell in every dimension.
    subroutine splpak_integrate(me,ndim,lower,upper,coef,xmin,xmax,nodes,value,ierror)
        class(splpak_type),intent(inout) :: me
        integer,intent(in) :: ndim
        real(wp),intent(in) :: lower(*), upper(*)
        real(wp),intent(in),target :: coef(*)
        real(wp),intent(in),target :: xmin(*), xmax(*)
        integer,intent(in),target :: nodes(*)
        real(wp),intent(out) :: value
        integer,intent(out) :: ierror
        real(wp),target :: ax(2*max(ndim,1)), f1(1)
        integer :: one(max(ndim,1)), idim
        one = 1
        ax = 0.0_wp
        do idim = 1, ndim
            ax(2*idim-1) = lower(idim)
            ax(2*idim) = upper(idim)
        end do
        f1 = 0.0_wp
        call splpak_integrate_grid(me,ndim,one,one,ax,coef,xmin,xmax,nodes,f1,ierror)
        value = f1(1)
    end subroutine splpak_integrate

    !> Several coefficient sets at the same batch of points -- the evaluation half of `refit`: f(i,k) is the spline of
    !! coef(:,k) (with `nderiv`, that partial derivative) at x(:,i), the very value `evaluate_many` returns for that field.
    !! coef is coef(ldcoef,nfields) as `refit` fills it, f is f(ldf,nfields) with ldf >= nq; rows of f beyond nq are not
    !! touched.  One call of the HIP library (splpak_eval_fields_f64: coordinates read, factor tables built and, for large
    !! batches, queries sorted once for all fields); under set_host(.true.), in the -DREAL128 build, for ndim > 4 or with
    !! SPLPAK_HOST_IF_NO_GPU=1 the module's host evaluation field by field, as in evaluate_many.
    !! ierror: 101..104 as splde (104: computed with nderiv clamped), -3 for nfields < 1, nq < 0 or a leading dimension too small.
    subroutine splpak_eval_fields(me,ndim,nq,x,ldx,nfields,coef,ldcoef,xmin,xmax,nodes,f,ldf,ierror,nderiv)
        class(splpak_type),intent(inout) :: me
        integer,intent(in) :: ndim, nq, ldx, nfields, ldcoef, ldf
        real(wp),intent(in),target :: x(ldx,*)
        real(wp),intent(in),target :: coef(ldcoef,*)
        real(wp),intent(in),target :: xmin(*), xmax(*)
        integer,intent(in),target :: nodes(*)
        real(wp),intent(inout),target :: f(ldf,*)
        integer,intent(out) :: ierror
        integer,intent(in),optional,target :: nderiv(*)
        integer(c_int32_t) :: rc
        integer :: k, ie, idim, ncol
        type(c_ptr) :: pd
        me%mdim = ndim
        rc = 0
        pd = c_null_ptr
        if (present(nderiv)) pd = c_loc(nderiv)
#ifndef REAL128
        if (.not. (host_takes(me,ndim) .and. ndim >= 1)) &
            rc = c_eval_fields(int(ndim,c_int32_t), int(nq,c_int64_t), c_loc(x), int(ldx,c_int32_t), pd, int(nfields,c_int32_t), &
                               c_loc(coef), int(ldcoef,c_int64_t), c_loc(xmin), c_loc(xmax), c_loc(nodes), c_loc(f), int(ldf,c_int64_t))
#endif
        if ((host_takes(me,ndim) .or. host_if_no_gpu(int(rc))) .and. ndim >= 1) then   ! host solver: evaluate_many's host loop per field
            ierror = 0
            ncol = 1
            do idim = 1, ndim
                ncol = ncol*max(nodes(idim),1)
            end do
            if (nfields < 1 .or. nq < 0 .or. ldf < nq .or. ldx < ndim .or. ldcoef < ncol) then
                ierror = -3
                call report(ierror,' evaluate_fields - NFIELDS < 1, NQ < 0 or a leading dimension is too small')
                return
            end if
            do k = 1, nfields
                call eval_common(me,ndim,int(nq,c_int64_t),c_loc(x),ldx,pd,c_loc(coef(1,k)),c_loc(xmin),c_loc(xmax), &
                                 c_loc(nodes),c_loc(f(1,k)),ie)
                if (ie /= 0) ierror = ie
                if (ie /= 0 .and. ie /= 104) return
            end do
            return
        end if
#ifdef REAL128
        rc = -1
#endif
        ierror = int(rc)
        select case (ierror)
        case (0)
        case (101); call report(ierror,' splfe or splde - NDIM is less than 1')
        case (102); call report(ierror,' splfe or splde - NODES(IDIM) is less than  4for some IDIM')
        case (103); call report(ierror,' splfe or splde - XMIN(IDIM) = XMAX(IDIM) for some IDIM')
        case (104); call report(ierror,' splde - NDERIV(IDIM) IS less than 0 or greater than 2 for some IDIM')
        case default
            if (ierror < 0) call report_library_failure(ierror,'evaluate_fields')
        end select
    end subroutine splpak_eval_fields

    subroutine eval_common(me,ndim,nq,x,ldx,nderiv,coef,xmin,xmax,nodes,f,ierror)
        class(splpak_type),intent(inout) :: me
        integer,intent(in) :: ndim, ldx
        integer(c_int64_t),intent(in) :: nq
        type(c_ptr),intent(in) :: x, nderiv, coef, xmin, xmax, nodes, f
        integer,intent(out) :: ierror
        integer(c_int32_t) :: rc
        real(wp),pointer :: px(:,:), pc(:), pmin(:), pmax(:), pf(:)
        integer,pointer :: pn(:), pd(:)
        integer :: iq, ie, zero(max(ndim,1)), ncol, idim
        me%mdim = ndim
        rc = 0
#ifndef REAL128
        if (.not. (host_takes(me,ndim) .and. ndim >= 1)) &
            rc = c_eval(int(ndim,c_int32_t), nq, x, int(ldx,c_int32_t), nderiv, coef, xmin, xmax, nodes, f)
#endif
        if ((host_takes(me,ndim) .or. host_if_no_gpu(int(rc))) .and. ndim >= 1) then   ! host solver: a loop over the scalar evaluation
            call c_f_pointer(nodes, pn, [ndim])
            ncol = 1
            do idim = 1, ndim
                ncol = ncol*max(pn(idim),1)
            end do
            call c_f_pointer(x, px, [ldx, int(nq)])
            call c_f_pointer(coef, pc, [ncol])
            call c_f_pointer(xmin, pmin, [ndim])
            call c_f_pointer(xmax, pmax, [ndim])
            call c_f_pointer(f, pf, [int(nq)])
            zero = 0
            ierror = 0
            do iq = 1, int(nq)
                if (c_associated(nderiv)) then
                    call c_f_pointer(nderiv, pd, [ndim])
                    pf(iq) = eval_point(me,ndim,px(:,iq),pd,pc,pmin,pmax,pn,ie)
                else
                    pf(iq) = eval_point(me,ndim,px(:,iq),zero,pc,pmin,pmax,pn,ie)
                end if
                if (ie /= 0) ierror = ie
                if (ie /= 0 .and. ie /= 104) return
            end do
            return
        end if
#ifdef REAL128
        rc = -1
#endif
        ierror = int(rc)
        select case (ierror)
        case (0)
        case (101); call report(ierror,' splfe or splde - NDIM is less than 1')
        case (102); call report(ierror,' splfe or splde - NODES(IDIM) is less than  4for some IDIM')
        case (103); call report(ierror,' splfe or splde - XMIN(IDIM) = XMAX(IDIM) for some IDIM')
        case (104); call report(ierror,' splde - NDERIV(IDIM) IS less than 0 or greater than 2 for some IDIM')
        case default
            if (ierror < 0) call report_library_failure(ierror,'splfe or splde')
        end select
    end subroutine eval_common

end module splpak_module
