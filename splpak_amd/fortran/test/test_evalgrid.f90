!> `evaluate_grid` of the drop-in module against its own scalar `evaluate` (the host computation that test_evalfix
!! holds to the reference's splde values, src/splpak.F90:1089-1240) at EVERY point of a tensor-product grid of points,
!! on the node grids and coefficients of the golden fixtures tests/golden/eval_<case>.txt (only their headers and
!! coefficients are read).  Axes are unsorted and hold xmin, xmax, a node position, a repeated value and points outside
!! the box.  With `host` as first argument the object runs under set_host(.true.) and the bar is 1e-12 (no GPU needed);
!! without it the grid call runs on the GPU (more than four dimensions: on the host, by the module itself) and the bar
!! is 1e-10.   usage: test_evalgrid [host] <fixture.txt> [...]
program test_evalgrid
    use splpak_module, wp => splpak_wp
    implicit none
    integer :: nargs, ia, nbad, first
    logical :: host
    real(wp) :: tol
    character(len=1024) :: path

    nbad = 0
    host = .false.
    first = 1
    nargs = command_argument_count()
    if (nargs >= 1) then
        call get_command_argument(1, path)
        if (trim(path) == 'host') then
            host = .true.
            first = 2
        end if
    end if
    if (nargs < first) error stop 'usage: test_evalgrid [host] fixture.txt ...'
    tol = merge(1.0e-12_wp, 1.0e-10_wp, host)
    do ia = first, nargs
        call get_command_argument(ia, path)
        call one(trim(path))
    end do
    if (nbad /= 0) error stop 'FAIL test_evalgrid'
    write(*,'(A)') ' PASS test_evalgrid'
contains
    subroutine one(file)
        character(len=*),intent(in) :: file
        integer :: u, ndim, ncol, npat, nqf, k, j, ip, ierror, seed, iq, nq, idim
        integer :: nodes(8), npts(8), nder(8), off(8), kk(8)
        real(wp) :: xmin(8), xmax(8), x(8), w, v, vmax, worst, cmax, scale
        real(wp),allocatable :: coef(:), axes(:), f(:), fs(:)
        type(splpak_type) :: s
        open(newunit=u, file=file, status='old', action='read')
        read(u,*) ndim
        read(u,*) nodes(1:ndim)
        read(u,*) xmin(1:ndim)
        read(u,*) xmax(1:ndim)
        read(u,*) ncol, npat, nqf
        allocate(coef(ncol))
        do k = 1, ncol
            read(u,*) coef(k)
        end do
        close(u)
        if (host) call s%set_host(.true.)
        call s%destroy(ndim)
        ! odd counts, more points along the first dimensions; small in 5-D
        do k = 1, ndim
            npts(k) = merge(11 - 2*k, 4 + mod(k,2), ndim <= 4)
        end do
        if (ndim == 3) npts(1) = 70             ! more than one workgroup tile along the first dimension
        nq = product(npts(1:ndim))
        allocate(axes(sum(npts(1:ndim))), f(nq), fs(nq))
        seed = 12345 + ndim
        j = 0
        do k = 1, ndim
            off(k) = j
            w = xmax(k) - xmin(k)
            do iq = 1, npts(k)
                seed = mod(seed*1103 + 12345, 65536)
                axes(j+iq) = xmin(k) - 0.15_wp*w + 1.3_wp*w*real(seed,wp)/65536.0_wp
            end do
            axes(j+1) = xmax(k)
            axes(j+2) = xmin(k) + (w/real(nodes(k)-1,wp))*real(nodes(k)/2,wp)     ! a node
            axes(j+npts(k)) = xmin(k)
            if (npts(k) >= 5) axes(j+4) = axes(j+3)                               ! a repeat
            j = j + npts(k)
        end do
        cmax = maxval(abs(coef))
        worst = 0.0_wp
        do ip = 0, 1
            nder = 0
            if (ip == 1) then
                do k = 1, ndim
                    nder(k) = mod(k,3)
                end do
            end if
            ! the scalar evaluation at every grid point, dimension 1 fastest
            kk = 1
            vmax = 0.0_wp
            do iq = 1, nq
                do idim = 1, ndim
                    x(idim) = axes(off(idim) + kk(idim))
                end do
                fs(iq) = s%evaluate(ndim, x(1:ndim), nder(1:ndim), coef, xmin(1:ndim), xmax(1:ndim), nodes(1:ndim), ierror)
                if (ierror /= 0) nbad = nbad + 1
                vmax = max(vmax, abs(fs(iq)))
                idim = 1
                do while (idim <= ndim)
                    kk(idim) = kk(idim) + 1
                    if (kk(idim) <= npts(idim)) exit
                    kk(idim) = 1
                    idim = idim + 1
                end do
            end do
            ! scale = the size of the terms that are summed (as test_evalfix)
            scale = cmax
            do k = 1, ndim
                scale = scale * (real(nodes(k) - 1, wp)/(xmax(k) - xmin(k)))**nder(k)
            end do
            vmax = max(vmax, scale)
            f = -huge(1.0_wp)
            if (ip == 0) then
                call s%evaluate_grid(ndim, npts(1:ndim), axes, coef, xmin(1:ndim), xmax(1:ndim), nodes(1:ndim), f, ierror)
            else
                call s%evaluate_grid(ndim, npts(1:ndim), axes, coef, xmin(1:ndim), xmax(1:ndim), nodes(1:ndim), f, ierror, &
                                     nderiv=nder(1:ndim))
            end if
            if (ierror /= 0) then
                nbad = nbad + 1
                write(*,*) 'ierror ', ierror, ' pattern ', ip
            end if
            do iq = 1, nq
                v = abs(f(iq) - fs(iq))
                worst = max(worst, v/max(vmax, tiny(1.0_wp)))
                if (.not. (v <= tol*vmax)) then
                    nbad = nbad + 1
                    if (nbad < 10) write(*,'(A,I3,A,I8,2ES25.16)') ' mismatch: pattern ', ip, ' point ', iq, f(iq), fs(iq)
                end if
            end do
        end do
        write(*,'(A,A,A,I8,A,ES10.2)') ' ', file, ': 2 patterns x ', nq, ' grid points, worst relative difference ', worst
    end subroutine one
end program test_evalgrid
