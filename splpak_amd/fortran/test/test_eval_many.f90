!> `evaluate_each` and `residuals_each` of the drop-in module: a batch of three 1-D problems of 40, 90 and 25 points on 9 nodes
!! with an empty problem among them, fitted by `initialize_many` with weights of which some are 0.
!!  * evaluate_each against `evaluate_many` on every problem alone with that problem's coefficients (the same bits: the library's
!!    promise) and against `evaluate` point by point (the host computation in the reference's order of summation, which differs
!!    by rounding: 1e-10 of the largest value, the project's parity bar); a derivative pattern the same way; entries of f
!!    outside the batch untouched;
!!  * residuals_each: resid = y - f, and stats(2,k) reproduced by a loop in the stated order -- 64 strided partial sums, product
!!    and sum rounded on their own (the product goes through a volatile), then the butterfly 32 .. 1 -- bit for bit in the
!!    double precision build; the count, the maximum and its zero-based index from the residuals;
!!  * the refusal of both under set_host.   usage: test_eval_many
program test_eval_many
    use splpak_module, wp => splpak_wp
    use, intrinsic :: iso_c_binding, only: c_int64_t, c_double
    implicit none
    integer,parameter :: nodes(1) = [9], ncol = 9, nbatch = 4, ntot = 40 + 90 + 25, pad = 3
    real(wp),parameter :: xmin(1) = [0.0_wp], xmax(1) = [1.0_wp]
    integer(c_int64_t) :: offsets(nbatch+1)
    real(wp) :: x(1,ntot+pad), y(ntot+pad), w(ntot+pad), coef(ncol,nbatch), f(ntot+pad), f1(ntot), fd(ntot+pad), resid(ntot+pad)
    real(wp) :: fp, worst, scale, tol
    real(c_double) :: stats(4,nbatch), lanes(0:63), tmp(0:63), t, amax
    real(c_double),volatile :: tt
    integer :: ierrors(nbatch), ierror, k, ip, i0, n, seed, nbad, l, o, p, cnt, imax
    type(splpak_type) :: s, q, h

    tol = 1.0e-10_wp
    nbad = 0
    seed = 9173
    offsets = [0_c_int64_t, 40_c_int64_t, 40_c_int64_t, 130_c_int64_t, 155_c_int64_t]      ! problem 2 is empty
    do ip = 1, ntot + pad
        x(1,ip) = -0.1_wp + 1.2_wp*lcg()
        y(ip) = sin(3.0_wp*x(1,ip)) + 0.05_wp*(lcg() - 0.5_wp)
        w(ip) = 0.5_wp + 1.5_wp*lcg()
        if (lcg() < 0.15_wp .and. ip /= 1 .and. ip /= 41 .and. ip /= 131) w(ip) = 0.0_wp
    end do
    coef = -7.0_wp
    call s%initialize_many(1, nbatch, offsets, x, 1, y, xmin, xmax, nodes, 1.0_wp, coef, ncol, ierrors, ierror, wdata=w)
    if (ierror /= 105) nbad = nbad + 1

    ! evaluate_each: values, then the first derivative
    f = -7.0_wp
    fd = -7.0_wp
    call s%evaluate_each(1, nbatch, offsets, x, 1, coef, ncol, xmin, xmax, nodes, f, ierror)
    if (ierror /= 0) nbad = nbad + 1
    call s%evaluate_each(1, nbatch, offsets, x, 1, coef, ncol, xmin, xmax, nodes, fd, ierror, nderiv=[1])
    if (ierror /= 0) nbad = nbad + 1
    if (any(f(ntot+1:) /= -7.0_wp) .or. any(fd(ntot+1:) /= -7.0_wp)) nbad = nbad + 1
    do k = 1, nbatch
        n = int(offsets(k+1) - offsets(k))
        if (n == 0) cycle
        i0 = int(offsets(k)) + 1
        call q%evaluate_many(1, n, x(:,i0:i0+n-1), 1, coef(:,k), xmin, xmax, nodes, f1, ierror)
        if (ierror /= 0 .or. any(f1(1:n) /= f(i0:i0+n-1))) nbad = nbad + 1
        call q%evaluate_many(1, n, x(:,i0:i0+n-1), 1, [1], coef(:,k), xmin, xmax, nodes, f1, ierror)
        if (ierror /= 0 .or. any(f1(1:n) /= fd(i0:i0+n-1))) nbad = nbad + 1
        worst = 0.0_wp
        scale = maxval(abs(f(i0:i0+n-1)))
        do ip = i0, i0 + n - 1
            fp = q%evaluate(1, x(:,ip), coef(:,k), xmin, xmax, nodes, ierror)
            if (ierror /= 0) nbad = nbad + 1
            worst = max(worst, abs(fp - f(ip))/scale)
        end do
        if (.not. (worst <= tol)) nbad = nbad + 1
        write(*,'(A,I2,A,I4,A,ES10.2)') ' problem ', k, ': ', n, ' points, evaluate_each vs evaluate point by point ', worst
    end do
    call s%evaluate_each(1, nbatch, offsets, x, 1, coef, ncol, xmin, xmax, nodes, f1, ierror, nderiv=[3])
    if (ierror /= 104) nbad = nbad + 1

    ! residuals_each
    resid = -7.0_wp
    stats = -7.0_c_double
    call s%residuals_each(1, nbatch, offsets, x, 1, y, coef, ncol, xmin, xmax, nodes, resid, stats, ierror, wdata=w)
    if (ierror /= 0) nbad = nbad + 1
    if (any(resid(ntot+1:) /= -7.0_wp)) nbad = nbad + 1
    if (kind(1.0_wp) == c_double) then
        if (any(resid(1:ntot) /= y(1:ntot) - f(1:ntot))) nbad = nbad + 1
    end if
    do k = 1, nbatch
        n = int(offsets(k+1) - offsets(k))
        i0 = int(offsets(k)) + 1
        lanes = 0.0_c_double
        cnt = 0
        amax = -1.0_c_double
        imax = -1
        do p = 0, n - 1          ! (ascending p: every lane l = mod(p, 64) sees its points in ascending order)
            if (w(i0+p) == 0.0_wp) cycle
            l = mod(p, 64)
            t = real(w(i0+p), c_double)*real(resid(i0+p), c_double)
            tt = t*t
            lanes(l) = lanes(l) + tt
            cnt = cnt + 1
            if (abs(t) > amax) then
                amax = abs(t)
                imax = p
            end if
        end do
        o = 32
        do while (o > 0)
            do l = 0, 63
                tmp(l) = lanes(l) + lanes(ieor(l, o))
            end do
            lanes = tmp
            o = o/2
        end do
        if (cnt == 0) amax = 0.0_c_double
        if (stats(1,k) /= real(cnt, c_double) .or. stats(4,k) /= real(imax, c_double)) nbad = nbad + 1
        if (kind(1.0_wp) == c_double) then
            if (stats(2,k) /= lanes(0) .or. stats(3,k) /= amax) nbad = nbad + 1
        else      ! (single precision storage: the unrounded residuals are not available to this loop)
            if (abs(stats(2,k) - lanes(0)) > 1.0e-5_c_double*lanes(0) .or. abs(stats(3,k) - amax) > 1.0e-5_c_double*amax) nbad = nbad + 1
        end if
        write(*,'(A,I2,A,I4,A,ES23.16,A,ES23.16)') ' problem ', k, ': counted ', cnt, ', S ', stats(2,k), ' restated ', lanes(0)
    end do
    if (any(stats(:,2) /= [0.0_c_double, 0.0_c_double, 0.0_c_double, -1.0_c_double])) nbad = nbad + 1
    if (.not. (stats(1,3) < 90.0_c_double .and. stats(1,1) + stats(1,3) + stats(1,4) < real(ntot, c_double))) nbad = nbad + 1      ! (zero weights)

    ! the argument checks are the library's; under set_host both refuse
    call s%residuals_each(1, nbatch, offsets, x, 1, y, coef, ncol - 1, xmin, xmax, nodes, resid, stats, ierror)
    if (ierror /= 104) nbad = nbad + 1
    call h%set_host(.true.)
    call h%evaluate_each(1, nbatch, offsets, x, 1, coef, ncol, xmin, xmax, nodes, f, ierror)
    if (ierror /= -4) nbad = nbad + 1
    call h%residuals_each(1, nbatch, offsets, x, 1, y, coef, ncol, xmin, xmax, nodes, resid, stats, ierror)
    if (ierror /= -4) nbad = nbad + 1
    if (nbad /= 0) error stop 'FAIL test_eval_many'
    write(*,'(A)') ' PASS test_eval_many'
contains
    real(wp) function lcg()
        seed = mod(seed*1103 + 12345, 65536)
        lcg = real(seed, wp)/65536.0_wp
    end function lcg
end program test_eval_many
