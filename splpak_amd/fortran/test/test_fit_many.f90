!> `initialize_many` of the drop-in module: a batch of three 1-D problems of 40, 90 and 25 points on 9 nodes, with an empty
!! problem among them, xtrap = 1, the second with weights of which some are 0 -- each compared with `initialize` on that problem
!! alone at 1e-10; then the statuses of the empty problem and of a problem that has too few points at xtrap = 0, and the
!! refusal under set_host.   usage: test_fit_many
program test_fit_many
    use splpak_module, wp => splpak_wp
    use, intrinsic :: iso_c_binding, only: c_int64_t
    implicit none
    integer,parameter :: nodes(1) = [9], ncol = 9, nbatch = 4, ntot = 40 + 90 + 25
    real(wp),parameter :: xmin(1) = [0.0_wp], xmax(1) = [1.0_wp]
    integer(c_int64_t) :: offsets(nbatch+1)
    real(wp) :: x(1,ntot), y(ntot), w(ntot), coef(ncol,nbatch), c1(ncol), work(ncol+8), worst, tol
    integer :: ierrors(nbatch), ierror, k, ip, i0, n, seed, nbad
    type(splpak_type) :: s, p, h

    tol = 1.0e-10_wp
    nbad = 0
    seed = 9173
    offsets = [0_c_int64_t, 40_c_int64_t, 40_c_int64_t, 130_c_int64_t, 155_c_int64_t]      ! problem 2 is empty
    do ip = 1, ntot
        x(1,ip) = -0.1_wp + 1.2_wp*lcg()
        y(ip) = sin(3.0_wp*x(1,ip)) + 0.05_wp*(lcg() - 0.5_wp)
        w(ip) = 0.5_wp + 1.5_wp*lcg()
        if (lcg() < 0.15_wp .and. ip /= 1 .and. ip /= 41 .and. ip /= 131) w(ip) = 0.0_wp
    end do
    coef = -7.0_wp
    call s%initialize_many(1, nbatch, offsets, x, 1, y, xmin, xmax, nodes, 1.0_wp, coef, ncol, ierrors, ierror, wdata=w)
    if (ierror /= 105) then
        nbad = nbad + 1
        write(*,*) 'initialize_many: ierror ', ierror
    end if
    if (ierrors(2) /= 105 .or. any(coef(:,2) /= -7.0_wp)) nbad = nbad + 1
    do k = 1, nbatch
        if (k == 2) cycle
        i0 = int(offsets(k)) + 1
        n = int(offsets(k+1) - offsets(k))
        if (ierrors(k) /= 0) nbad = nbad + 1
        call p%initialize(1, x(:,i0:i0+n-1), 1, y(i0:i0+n-1), w(i0:i0+n-1), n, xmin, xmax, nodes, 1.0_wp, c1, ncol, work, ncol+8, ierror)
        if (ierror /= 0) nbad = nbad + 1
        worst = maxval(abs(coef(:,k) - c1))/maxval(abs(c1))
        if (.not. (worst <= tol)) nbad = nbad + 1
        write(*,'(A,I2,A,I4,A,ES10.2)') ' problem ', k, ': ', n, ' points, worst relative difference ', worst
    end do
    ! without weights (splcc), and a problem of two points at xtrap = 0: 107 for it alone, its coefficients zeroed
    offsets(1:3) = [0_c_int64_t, 40_c_int64_t, 42_c_int64_t]
    call s%initialize_many(1, 2, offsets, x, 1, y, xmin, xmax, nodes, 0.0_wp, coef, ncol, ierrors, ierror)
    if (ierror /= 107 .or. ierrors(1) /= 0 .or. ierrors(2) /= 107 .or. any(coef(:,2) /= 0.0_wp)) nbad = nbad + 1
    call p%initialize(1, x(:,1:40), 1, y(1:40), 40, xmin, xmax, nodes, 0.0_wp, c1, ncol, work, ncol+8, ierror)
    if (ierror /= 0) nbad = nbad + 1
    worst = maxval(abs(coef(:,1) - c1))/maxval(abs(c1))
    if (.not. (worst <= tol)) nbad = nbad + 1
    write(*,'(A,ES10.2)') ' unweighted, xtrap = 0: worst relative difference ', worst
    ! the argument checks are the library's; under set_host the entry refuses
    call s%initialize_many(3, 2, offsets, x, 3, y, xmin, xmax, nodes, 0.0_wp, coef, ncol, ierrors, ierror)
    if (ierror /= -4) nbad = nbad + 1
    call h%set_host(.true.)
    call h%initialize_many(1, 2, offsets, x, 1, y, xmin, xmax, nodes, 0.0_wp, coef, ncol, ierrors, ierror)
    if (ierror /= -4) nbad = nbad + 1
    if (nbad /= 0) error stop 'FAIL test_fit_many'
    write(*,'(A)') ' PASS test_fit_many'
contains
    real(wp) function lcg()
        seed = mod(seed*1103 + 12345, 65536)
        lcg = real(seed, wp)/65536.0_wp
    end function lcg
end program test_fit_many
