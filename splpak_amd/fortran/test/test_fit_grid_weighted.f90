!> `initialize_grid_weighted` of the drop-in module against `initialize` on the listed samples of non-zero weight: a 3-D
!! sample of 18 x 15 x 13 points on 6 x 5 x 4 nodes, unsorted axes with a repeated value and a point outside the box on each,
!! xtrap = 0, a weight per sample -- a separable factor times a factor per sample in [0.5, 2], 15 % of the samples masked
!! (weight 0, value NaN).  Then `evaluate` on the object that `initialize_grid_weighted` left.  With `host` as argument the
!! object runs under set_host(.true.) -- the module lists the samples and calls its host solver -- and the bar is 1e-12 (no
!! GPU needed); without it the fit is one call of the HIP library and the bar is 1e-10.   usage: test_fit_grid_weighted [host]
program test_fit_grid_weighted
    use splpak_module, wp => splpak_wp
    use, intrinsic :: ieee_arithmetic, only: ieee_value, ieee_quiet_nan
    implicit none
    integer,parameter :: ndim = 3
    integer,parameter :: npts(ndim) = [18, 15, 13], nodes(ndim) = [6, 5, 4]
    integer,parameter :: nsamp = 18*15*13, ncol = 6*5*4, ntab = 18 + 15 + 13
    real(wp),parameter :: xmin(ndim) = [-1.25_wp, 0.0_wp, 2.0_wp], xmax(ndim) = [3.5_wp, 1.0_wp, 2.75_wp]
    logical :: host
    real(wp) :: tol, axes(ntab), waxes(ntab), values(nsamp), weights(nsamp), xl(ndim,nsamp), wl(nsamp), yl(nsamp)
    real(wp) :: cg(ncol), cp(ncol), work(1), x(ndim), xs(ndim), dx, u, worst, cmax, vg, vp, w
    integer :: k, j, ip, idim, seed, off(ndim), kk(ndim), ierror, nbad, nl
    character(len=64) :: arg
    type(splpak_type) :: s, p

    host = .false.
    if (command_argument_count() >= 1) then
        call get_command_argument(1, arg)
        host = trim(arg) == 'host'
    end if
    tol = merge(1.0e-12_wp, 1.0e-10_wp, host)
    if (host) then
        call s%set_host(.true.)
        call p%set_host(.true.)
    end if
    nbad = 0
    seed = 4712
    j = 0
    do k = 1, ndim
        off(k) = j
        dx = (xmax(k) - xmin(k))/real(nodes(k) - 1, wp)
        do ip = 1, npts(k)
            ! one coordinate per stratum of the box, jittered, in a scrambled order (7 is prime to 18, 15 and 13)
            u = (real(mod(7*ip, npts(k)), wp) + 0.1_wp + 0.8_wp*lcg())/real(npts(k), wp)
            axes(j+ip) = xmin(k) + u*(xmax(k) - xmin(k))
            waxes(j+ip) = 0.5_wp + 1.5_wp*lcg()
        end do
        axes(j+2) = axes(j+1)                          ! a repeat
        axes(j+3) = xmax(k) + 0.4_wp*dx                ! outside the box
        axes(j+4) = xmin(k) + 2.0_wp*dx                ! a node
        j = j + npts(k)
    end do
    kk = 1
    nl = 0
    do ip = 1, nsamp
        w = 0.5_wp + 1.5_wp*lcg()
        do idim = 1, ndim
            xs(idim) = axes(off(idim) + kk(idim))
            w = w*waxes(off(idim) + kk(idim))
        end do
        values(ip) = sin(1.3_wp*xs(1))*cos(2.1_wp*xs(2)) + 0.5_wp*xs(3) + 0.05_wp*(lcg() - 0.5_wp)
        if (lcg() < 0.15_wp) then                      ! masked: never read
            weights(ip) = 0.0_wp
            values(ip) = ieee_value(1.0_wp, ieee_quiet_nan)
        else
            weights(ip) = w
            nl = nl + 1
            xl(:,nl) = xs
            wl(nl) = w
            yl(nl) = values(ip)
        end if
        idim = 1
        do while (idim <= ndim)
            kk(idim) = kk(idim) + 1
            if (kk(idim) <= npts(idim)) exit
            kk(idim) = 1
            idim = idim + 1
        end do
    end do

    cg = -huge(1.0_wp)
    call s%initialize_grid_weighted(ndim, npts, axes, values, weights, xmin, xmax, nodes, 0.0_wp, cg, ncol, ierror)
    if (ierror /= 0) then
        nbad = nbad + 1
        write(*,*) 'initialize_grid_weighted: ierror ', ierror
    end if
    call p%initialize(ndim, xl, ndim, yl, wl, nl, xmin, xmax, nodes, 0.0_wp, cp, ncol, work, 1, ierror)
    if (ierror /= 0) then
        nbad = nbad + 1
        write(*,*) 'initialize: ierror ', ierror
    end if
    cmax = maxval(abs(cp))
    worst = maxval(abs(cg - cp))/cmax
    if (.not. (worst <= tol)) nbad = nbad + 1
    write(*,'(A,I6,A,I6,A,I4,A,ES10.2)') ' ', nl, ' of ', nsamp, ' samples, ', ncol, &
        ' coefficients, worst relative difference ', worst
    ! the object is as `initialize` leaves it: the scalar evaluation follows
    x = 0.5_wp*(xmin + xmax)
    vg = s%evaluate(ndim, x, cg, xmin, xmax, nodes, ierror)
    if (ierror /= 0) nbad = nbad + 1
    vp = p%evaluate(ndim, x, cp, xmin, xmax, nodes, ierror)
    if (ierror /= 0) nbad = nbad + 1
    if (.not. (abs(vg - vp) <= 64.0_wp*tol*cmax)) nbad = nbad + 1
    ! the argument checks are `initialize`'s: an axis without points
    call s%initialize_grid_weighted(ndim, [18, 0, 13], axes, values, weights, xmin, xmax, nodes, 0.0_wp, cg, ncol, ierror)
    if (ierror /= 105) nbad = nbad + 1
    ! a negative weight is refused
    weights(5) = -1.0_wp
    call s%initialize_grid_weighted(ndim, npts, axes, values, weights, xmin, xmax, nodes, 0.0_wp, cg, ncol, ierror)
    if (ierror /= -3) nbad = nbad + 1
    if (nbad /= 0) error stop 'FAIL test_fit_grid_weighted'
    write(*,'(A)') ' PASS test_fit_grid_weighted'
contains
    real(wp) function lcg()
        seed = mod(seed*1103 + 12345, 65536)
        lcg = real(seed, wp)/65536.0_wp
    end function lcg
end program test_fit_grid_weighted
