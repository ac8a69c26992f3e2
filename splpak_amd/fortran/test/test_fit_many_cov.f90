!> `initialize_many_cov` and `variance_each` of the drop-in module: a batch of two weighted 1-D problems of 40 and 60 points on 9
!! nodes at xtrap = 0 (no constraint rows: Z is the covariance of the coefficients) with an empty problem between them.
!!  * coef and ierrors are those of `initialize_many`, bit for bit; the empty problem keeps its cov;
!!  * cov against a dense inverse formed in the program: the rows a(x_i) are `evaluate` of the nine unit coefficient vectors,
!!    N = sum_i w_i^2 a a^T, inverted by Gauss-Jordan steps on the symmetric positive definite matrix (no pivoting needed);
!!    every stencil entry within tol sqrt(Z_ii Z_jj), the slots outside the grid exactly 0;
!!  * variance_each against a^T Z a with that inverse, values and the first derivative, and sum_i w_i^2 v_i = 9 (the trace of
!!    the hat matrix); entries of v outside the batch untouched;
!!  * ldcov too small is 104; both refuse under set_host.
!! tol = 1e6 epsilon: the scaled condition number of these problems is below 1e4, and both inverses carry a few epsilon times it.
!! usage: test_fit_many_cov
program test_fit_many_cov
    use splpak_module, wp => splpak_wp
    use, intrinsic :: iso_c_binding, only: c_int64_t
    implicit none
    integer,parameter :: nodes(1) = [9], ncol = 9, hst = 4, nbatch = 3, ntot = 100, pad = 3, ldcov = ncol*hst + 2
    real(wp),parameter :: xmin(1) = [0.0_wp], xmax(1) = [1.0_wp]
    integer(c_int64_t) :: offsets(nbatch+1)
    real(wp) :: x(1,ntot+pad), y(ntot+pad), w(ntot+pad), coef(ncol,nbatch), coef0(ncol,nbatch), cov(ldcov,nbatch)
    real(wp) :: v(ntot+pad), vd(ntot+pad), a(ncol), ad(ncol), unit(ncol), nmat(ncol,ncol), z(ncol,ncol), want, tol, worst, trace, piv
    integer :: ierrors(nbatch), ierrors0(nbatch), ierror, k, ip, i0, n, seed, nbad, i, j, code, r
    type(splpak_type) :: s, q, h

    tol = 1.0e6_wp*epsilon(1.0_wp)
    nbad = 0
    seed = 4711
    offsets = [0_c_int64_t, 40_c_int64_t, 40_c_int64_t, 100_c_int64_t]      ! problem 2 is empty
    do ip = 1, ntot + pad
        x(1,ip) = lcg()
        y(ip) = sin(3.0_wp*x(1,ip)) + 0.05_wp*(lcg() - 0.5_wp)
        w(ip) = 0.5_wp + 1.5_wp*lcg()
    end do
    ! points in every cell, so that neither problem is rank deficient at xtrap = 0
    do ip = 1, 8
        x(1,ip) = (real(ip, wp) - 0.5_wp)/8.0_wp
        x(1,40+ip) = (real(ip, wp) - 0.3_wp)/8.0_wp
    end do
    x(1,9) = 0.0_wp; x(1,10) = 1.0_wp; x(1,49) = 0.0_wp; x(1,50) = 1.0_wp
    coef0 = -7.0_wp
    coef = -7.0_wp
    cov = -7.0_wp
    call s%initialize_many(1, nbatch, offsets, x, 1, y, xmin, xmax, nodes, 0.0_wp, coef0, ncol, ierrors0, ierror, wdata=w)
    if (ierror /= 105) nbad = nbad + 1
    call s%initialize_many_cov(1, nbatch, offsets, x, 1, y, xmin, xmax, nodes, 0.0_wp, coef, ncol, cov, ldcov, ierrors, ierror, wdata=w)
    if (ierror /= 105 .or. any(ierrors /= ierrors0) .or. any(ierrors /= [0, 105, 0])) nbad = nbad + 1
    if (any(coef /= coef0)) nbad = nbad + 1
    if (any(cov(:,2) /= -7.0_wp) .or. any(cov(ncol*hst+1:,:) /= -7.0_wp)) nbad = nbad + 1

    v = -7.0_wp
    vd = -7.0_wp
    call s%variance_each(1, nbatch, offsets, x, 1, cov, ldcov, xmin, xmax, nodes, v, ierror)
    if (ierror /= 0) nbad = nbad + 1
    call s%variance_each(1, nbatch, offsets, x, 1, cov, ldcov, xmin, xmax, nodes, vd, ierror, nderiv=[1])
    if (ierror /= 0) nbad = nbad + 1
    if (any(v(ntot+1:) /= -7.0_wp) .or. any(vd(ntot+1:) /= -7.0_wp)) nbad = nbad + 1

    do k = 1, nbatch
        n = int(offsets(k+1) - offsets(k))
        if (n == 0) cycle
        i0 = int(offsets(k)) + 1
        nmat = 0.0_wp
        do ip = i0, i0 + n - 1
            call row(x(:,ip), [0], a)
            do j = 1, ncol
                nmat(:,j) = nmat(:,j) + (w(ip)*a)*(w(ip)*a(j))
            end do
        end do
        ! z = nmat^-1 by Gauss-Jordan steps
        z = 0.0_wp
        do i = 1, ncol
            z(i,i) = 1.0_wp
        end do
        do i = 1, ncol
            piv = nmat(i,i)
            nmat(i,:) = nmat(i,:)/piv
            z(i,:) = z(i,:)/piv
            do r = 1, ncol
                if (r == i) cycle
                piv = nmat(r,i)
                nmat(r,:) = nmat(r,:) - piv*nmat(i,:)
                z(r,:) = z(r,:) - piv*z(i,:)
            end do
        end do
        worst = 0.0_wp
        do i = 1, ncol
            do code = 0, hst - 1
                j = i + code - 3
                if (j < 1) then
                    if (cov((i-1)*hst + code + 1, k) /= 0.0_wp) nbad = nbad + 1
                else
                    worst = max(worst, abs(cov((i-1)*hst + code + 1, k) - z(i,j))/sqrt(z(i,i)*z(j,j)))
                end if
            end do
        end do
        if (.not. (worst <= tol)) nbad = nbad + 1
        write(*,'(A,I2,A,ES10.2)') ' problem ', k, ': cov against the dense inverse, worst scaled difference ', worst
        worst = 0.0_wp
        trace = 0.0_wp
        do ip = i0, i0 + n - 1
            call row(x(:,ip), [0], a)
            call row(x(:,ip), [1], ad)
            want = dot_product(a, matmul(z, a))
            worst = max(worst, abs(v(ip) - want)/(sum(abs(a)*sqrt(diag(z)))**2))
            want = dot_product(ad, matmul(z, ad))
            worst = max(worst, abs(vd(ip) - want)/(sum(abs(ad)*sqrt(diag(z)))**2))
            trace = trace + w(ip)**2*v(ip)
        end do
        if (.not. (worst <= tol)) nbad = nbad + 1
        if (.not. (abs(trace - real(ncol, wp)) <= tol*real(ncol, wp))) nbad = nbad + 1
        write(*,'(A,I2,A,ES10.2,A,F18.14)') ' problem ', k, ': variance_each against a^T Z a ', worst, ', sum w^2 v = ', trace
    end do

    call s%initialize_many_cov(1, nbatch, offsets, x, 1, y, xmin, xmax, nodes, 0.0_wp, coef, ncol, cov, ncol*hst - 1, ierrors, ierror)
    if (ierror /= 104) nbad = nbad + 1
    call h%set_host(.true.)
    call h%initialize_many_cov(1, nbatch, offsets, x, 1, y, xmin, xmax, nodes, 0.0_wp, coef, ncol, cov, ldcov, ierrors, ierror)
    if (ierror /= -4) nbad = nbad + 1
    call h%variance_each(1, nbatch, offsets, x, 1, cov, ldcov, xmin, xmax, nodes, v, ierror)
    if (ierror /= -4) nbad = nbad + 1
    if (nbad /= 0) error stop 'FAIL test_fit_many_cov'
    write(*,'(A)') ' PASS test_fit_many_cov'
contains
    real(wp) function lcg()
        seed = mod(seed*1103 + 12345, 65536)
        lcg = real(seed, wp)/65536.0_wp
    end function lcg

    !> the window row of the point xp for the derivative pattern nd: the spline of every unit coefficient vector
    subroutine row(xp, nd, arow)
        real(wp),intent(in) :: xp(1)
        integer,intent(in) :: nd(1)
        real(wp),intent(out) :: arow(ncol)
        integer :: jj, ie
        do jj = 1, ncol
            unit = 0.0_wp
            unit(jj) = 1.0_wp
            arow(jj) = q%evaluate(1, xp, nd, unit, xmin, xmax, nodes, ie)
            if (ie /= 0) nbad = nbad + 1
        end do
    end subroutine row

    function diag(m) result(d)
        real(wp),intent(in) :: m(ncol,ncol)
        real(wp) :: d(ncol)
        integer :: ii
        do ii = 1, ncol
            d(ii) = m(ii,ii)
        end do
    end function diag
end program test_fit_many_cov
