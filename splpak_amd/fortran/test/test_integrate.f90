!> `integrate_grid` and `integrate` of the drop-in module against a quadrature over its own scalar `evaluate` (the host
!! computation that test_evalfix holds to the reference's splfe values, src/splpak.F90:1258-1275), on the node grids and
!! coefficients of the golden fixtures tests/golden/eval_<case>.txt (only their headers and coefficients are read).
!! The yardstick is formed here, apart from the module: every cell is cut at the node lines strictly inside it, each piece
!! gets two Gauss-Legendre points per dimension, `evaluate` runs at the tensor of them and the values are summed with the
!! product weights.  The fit is a cubic on every node cell and a straight line outside the grid, so the rule is exact.
!! Edges are unsorted and hold xmin, xmax, a node position, a repeated value (an empty cell), reversed cells and points
!! outside the box.  Every grid is integrated in all dimensions and with every second dimension evaluated (mode 0).
!! The error is measured against S = the largest sum over a cell of |weight * value|.  With `host` as first argument
!! the object runs under set_host(.true.) and the bar is 1e-12 (no GPU needed); without it the call runs on the GPU (more
!! than four dimensions: on the host, by the module itself) and the bar is 1e-10.  `integrate` over the first cell must
!! equal `integrate_grid` with that one cell to the bit.   usage: test_integrate [host] <fixture.txt> [...]
program test_integrate
    use splpak_module, wp => splpak_wp
    implicit none
    integer :: nargs, ia, nbad, first
    logical :: host
    real(wp) :: tol
    character(len=1024) :: path
    ! the grid, the coefficients and the axes of the case at hand (shared by `one` and its yardstick)
    integer :: nodes(8), mode(8), off(8), nder(8)
    real(wp) :: xmin(8), xmax(8)
    real(wp),allocatable :: coef(:), axes(:)
    type(splpak_type) :: s

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
    if (nargs < first) error stop 'usage: test_integrate [host] fixture.txt ...'
    tol = merge(1.0e-12_wp, 1.0e-10_wp, host)
    do ia = first, nargs
        call get_command_argument(ia, path)
        call one(trim(path))
    end do
    if (nbad /= 0) error stop 'FAIL test_integrate'
    write(*,'(A)') ' PASS test_integrate'
contains
    subroutine one(file)
        character(len=*),intent(in) :: file
        integer :: u, ndim, ncol, npat, nqf, k, j, ip, ierror, seed, iq, nq, idim, ne
        integer :: ncell(8), kk(8), ones(8)
        real(wp) :: lower(8), upper(8), w, v, s1, smax, worst, ref, mag, value
        real(wp),allocatable :: f(:), box(:)
        real(wp) :: g1(1)
        open(newunit=u, file=file, status='old', action='read')
        read(u,*) ndim
        read(u,*) nodes(1:ndim)
        read(u,*) xmin(1:ndim)
        read(u,*) xmax(1:ndim)
        read(u,*) ncol, npat, nqf
        if (allocated(coef)) deallocate(coef, axes)
        allocate(coef(ncol))
        do k = 1, ncol
            read(u,*) coef(k)
        end do
        close(u)
        if (host) call s%set_host(.true.)
        call s%destroy(ndim)
        nder = 0
        ones = 1
        do k = 1, ndim
            ncell(k) = merge(6 - k, 2, ndim <= 4)
        end do
        if (ndim == 3) ncell(1) = 70             ! more than one workgroup tile along the first dimension
        nq = product(ncell(1:ndim))
        allocate(axes(sum(ncell(1:ndim)) + ndim), f(nq), box(2*ndim))
        worst = 0.0_wp
        do ip = 0, 1
            mode = 1
            if (ip == 1) then
                do k = 2, ndim, 2
                    mode(k) = 0
                end do
            end if
            seed = 4321 + ndim + 100*ip
            j = 0
            do k = 1, ndim
                off(k) = j
                ne = ncell(k) + mode(k)
                w = xmax(k) - xmin(k)
                do iq = 1, ne
                    seed = mod(seed*1103 + 12345, 65536)
                    axes(j+iq) = xmin(k) - 0.15_wp*w + 1.3_wp*w*real(seed,wp)/65536.0_wp
                end do
                axes(j+1) = xmax(k)
                axes(j+2) = xmin(k) + (w/real(nodes(k)-1,wp))*real(nodes(k)/2,wp)     ! a node
                axes(j+ne) = xmin(k)
                if (ne >= 5) axes(j+4) = axes(j+3)                                    ! a repeat: cell 3 is empty
                j = j + ne
            end do
            f = -huge(1.0_wp)
            call s%integrate_grid(ndim, ncell(1:ndim), mode(1:ndim), axes, coef, xmin(1:ndim), xmax(1:ndim), nodes(1:ndim), &
                                  f, ierror)
            if (ierror /= 0) then
                nbad = nbad + 1
                write(*,*) 'ierror ', ierror, ' pattern ', ip
            end if
            ! the yardstick at every cell, dimension 1 fastest; S first, then the comparison
            smax = 0.0_wp
            do j = 1, 2
                kk = 1
                do iq = 1, nq
                    call cell_reference(ndim, kk, ref, mag)
                    if (j == 1) then
                        smax = max(smax, mag)
                    else
                        v = abs(f(iq) - ref)
                        worst = max(worst, v/max(smax, tiny(1.0_wp)))
                        if (.not. (v <= tol*smax)) then
                            nbad = nbad + 1
                            if (nbad < 10) write(*,'(A,I3,A,I8,2ES25.16)') ' mismatch: pattern ', ip, ' cell ', iq, f(iq), ref
                        end if
                    end if
                    idim = 1
                    do while (idim <= ndim)
                        kk(idim) = kk(idim) + 1
                        if (kk(idim) <= ncell(idim)) exit
                        kk(idim) = 1
                        idim = idim + 1
                    end do
                end do
            end do
            if (ip == 0) then
                ! an empty cell is exactly 0
                if (ncell(1) >= 4) then
                    if (f(3) /= 0.0_wp) then
                        nbad = nbad + 1
                        write(*,*) 'the empty cell is not 0: ', f(3)
                    end if
                end if
                ! `integrate` over the first cell: the bits of integrate_grid with that one cell, and the negation when one
                ! dimension is taken the other way round
                do k = 1, ndim
                    lower(k) = axes(off(k)+1)
                    upper(k) = axes(off(k)+2)
                    box(2*k-1) = lower(k)
                    box(2*k) = upper(k)
                end do
                call s%integrate(ndim, lower(1:ndim), upper(1:ndim), coef, xmin(1:ndim), xmax(1:ndim), nodes(1:ndim), value, ierror)
                if (ierror /= 0) nbad = nbad + 1
                call s%integrate_grid(ndim, ones(1:ndim), ones(1:ndim), box, coef, xmin(1:ndim), xmax(1:ndim), nodes(1:ndim), &
                                      g1, ierror)
                if (ierror /= 0) nbad = nbad + 1
                if (value /= g1(1)) then
                    nbad = nbad + 1
                    write(*,'(A,2ES25.16)') ' integrate differs from integrate_grid with one cell: ', value, g1(1)
                end if
                s1 = lower(1)
                lower(1) = upper(1)
                upper(1) = s1
                call s%integrate(ndim, lower(1:ndim), upper(1:ndim), coef, xmin(1:ndim), xmax(1:ndim), nodes(1:ndim), s1, ierror)
                if (ierror /= 0 .or. s1 /= -value) then
                    nbad = nbad + 1
                    write(*,'(A,2ES25.16)') ' a reversed box is not the negation: ', s1, value
                end if
            end if
        end do
        write(*,'(A,A,A,I8,A,ES10.2)') ' ', file, ': 2 patterns x ', nq, ' cells, worst relative difference ', worst
    end subroutine one

        !> the yardstick for the cell kk: sum of weight * evaluate over the tensor of the Gauss points of its pieces (ref) and
        !! the sum of the absolute terms (mag)
        subroutine cell_reference(ndim, kk, ref, mag)
            integer,intent(in) :: ndim, kk(*)
            real(wp),intent(out) :: ref, mag
            integer :: nqd(8), kq(8), idim, ie, ib, np
            real(wp) :: xq(2*66,8), wq(2*66,8), x(8), e0, e1, lo, hi, sgn, dx, bp, a, b, m, h, wt, v
            do idim = 1, ndim
                if (mode(idim) == 0) then
                    nqd(idim) = 1
                    xq(1,idim) = axes(off(idim) + kk(idim))
                    wq(1,idim) = 1.0_wp
                    cycle
                end if
                e0 = axes(off(idim) + kk(idim))
                e1 = axes(off(idim) + kk(idim) + 1)
                lo = min(e0,e1)
                hi = max(e0,e1)
                sgn = merge(1.0_wp, -1.0_wp, e1 >= e0)
                dx = (xmax(idim) - xmin(idim))/real(nodes(idim) - 1,wp)
                np = 0
                a = lo
                do ib = 0, nodes(idim)                  ! the node lines strictly inside, then the upper end
                    if (ib < nodes(idim)) then
                        bp = xmin(idim) + real(ib,wp)*dx
                        if (.not. (bp > a .and. bp < hi)) cycle
                        b = bp
                    else
                        b = hi
                    end if
                    m = 0.5_wp*(a + b)
                    h = 0.5_wp*(b - a)
                    xq(np+1,idim) = m - h/sqrt(3.0_wp)
                    xq(np+2,idim) = m + h/sqrt(3.0_wp)
                    wq(np+1,idim) = sgn*h
                    wq(np+2,idim) = sgn*h
                    np = np + 2
                    a = b
                end do
                nqd(idim) = np
            end do
            ref = 0.0_wp
            mag = 0.0_wp
            kq = 1
            do
                wt = 1.0_wp
                do idim = 1, ndim
                    x(idim) = xq(kq(idim),idim)
                    wt = wt*wq(kq(idim),idim)
                end do
                v = s%evaluate(ndim, x(1:ndim), nder(1:ndim), coef, xmin(1:ndim), xmax(1:ndim), nodes(1:ndim), ie)
                if (ie /= 0) nbad = nbad + 1
                ref = ref + wt*v
                mag = mag + abs(wt*v)
                idim = 1
                do while (idim <= ndim)
                    kq(idim) = kq(idim) + 1
                    if (kq(idim) <= nqd(idim)) exit
                    kq(idim) = 1
                    idim = idim + 1
                end do
                if (idim > ndim) exit
            end do
        end subroutine cell_reference
end program test_integrate
